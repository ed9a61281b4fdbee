"""Transitions between call shapes on ONE handle: how an encode call waits for the call before it depends on what both look like
(solo_enc_pipe.h: the same packets and chunks -> chunk by chunk; another length, a subset call, the other schedule -> for all of it;
asynchronous joins -> nothing but the handle's own events orders two calls).  The 25 packets of the golden batch on continued state in
calls of 1, 6, 6, 2, 7 and 3 packets: the 1-packet call is the one-chunk path, the second 6 follows an equal call (chunk-wise reuse of
the hand-over records), the 2-packet call is a subset call that lists every stream (map, verdict word and record layout change on both
sides of it), joins are asynchronous from the third call on.  Payload bytes and byte counts of every packet against the golden file,
under the default pipeline, chunks of 2 with a coder batch of 4, launch groups of 3 / 3 / 2 streams, and SOLO_ENC_PERSIST=1 (where
the persistent and the launch-per-chunk schedule alternate: calls of one packet and subset calls fall back)."""
import numpy as np
import pytest

import solo_testlib as T

pytestmark = pytest.mark.gpu

CALLS = (1, 6, 6, 2, 7, 3)
SUBSET_CALL, ASYNC_FROM = 3, 2
ENVS = [{}, {"SOLO_ENC_CHUNK": "2", "SOLO_ENC_RC_BATCH": "4"}, {"SOLO_ENC_GROUP": "3"}, {"SOLO_ENC_PERSIST": "1"}]


@pytest.mark.parametrize("env", ENVS, ids=["default", "chunk2_batch4", "group3", "persist"])
def test_call_shapes_in_turn_on_one_handle(monkeypatch, env):
    import torch
    import solo_amd
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    for key, v in env.items():
        monkeypatch.setenv(key, v)                                  # read when the handle first encodes
    z = np.load(T.GOLDEN + "/synth8x25.npz")
    N, P, S = z["bits"].shape
    assert (N, sum(CALLS)) == (8, P)
    b = solo_amd.SoloBatch(N, encoder=True, decoder=False, slot_bytes=S)
    ins, p0 = [], 0
    for n in CALLS:                                                 # inputs (and outputs) stay alive and untouched until wait_encode
        ins.append(torch.from_numpy(np.ascontiguousarray(z["pcm"][:, p0:p0 + n])).to(b.device))
        p0 += n
    torch.cuda.synchronize()
    outs = []
    for i, x in enumerate(ins):
        if i == ASYNC_FROM:
            b.set_async_join(True)
        outs.append(b.encode(x, streams=list(range(N)) if i == SUBSET_CALL else None))      # fresh output tensors per call
    b.wait_encode(1)
    b.wait_encode(0)
    torch.cuda.synchronize()
    for i, (_, _, st) in enumerate(outs):
        assert int(st.abs().max()) == 0, (i, st.cpu().numpy())
    bits = np.concatenate([o[0].cpu().numpy() for o in outs], axis=1)
    nb = np.concatenate([o[1].cpu().numpy() for o in outs], axis=1)
    assert np.array_equal(nb, z["nbytes"])
    for s in range(N):
        for p in range(P):
            n0 = int(nb[s, p, 0])
            assert np.array_equal(bits[s, p, :n0], z["bits"][s, p, :n0]), (s, p)
