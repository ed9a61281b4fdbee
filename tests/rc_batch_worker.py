"""The cases of tests/test_gpu_rc_batch.py and the child process that runs them: SOLO_ENC_RC_BATCH (packets per range-coder launch) is
read when a handle sets its pipeline up, so every knob value gets a fresh process.   python tests/rc_batch_worker.py KNOB K[,K..] out.npz

A case: one handle, a plan of state-continued encode calls over a fixed input.  What it leaves: payload slots (prefilled with 0xA5, so
the bytes no kernel may touch are compared too), byte counts and the status of every call."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

STREAMS = (1, 33, 65)          # a partial wavefront of the coder, a second workgroup of the one-launch-per-chunk coder, a third
FILL = 0xA5


def packets_of(k):
    return sorted({1, k - 1, k, k + 1, 2 * k + 3})


def plan(k, total):
    """calls of 2k+3, k+1, k, k-1 and 1 packets in turn until `total` packets are spent"""
    out, p, i = [], 0, 0
    sizes = [2 * k + 3, k + 1, k, k - 1, 1]
    while p < total:
        n = min(sizes[i % len(sizes)], total - p)
        out.append((p, n))
        p += n
        i += 1
    return out


def pcm_of(kind, n_streams, total):
    import refcodec as R
    import solo_testlib as T
    if kind == "speech":
        return np.stack([R.synth_stream(7100 + i, total) for i in range(n_streams)])
    if kind == "fs20":          # the same audio in packets of one 20 ms frame
        return np.stack([R.synth_stream(7100 + i, (total + 1) // 2).reshape(-1, 320)[:total] for i in range(n_streams)])
    if kind == "wb":
        return np.stack([T.synth_stream_32k(7100 + i, total) for i in range(n_streams)])
    if kind == "dtx":           # three packets of speech, then near-silence: the encoder goes into DTX a few packets later
        x = np.stack([R.synth_stream(7100 + i, total) for i in range(n_streams)])
        rng = np.random.default_rng(11)
        x[:, 3:] = (rng.standard_normal(x[:, 3:].shape) * 3).astype(np.int16)
        return x
    raise ValueError(kind)


def cases(k):
    """name -> dict(n, total, kind, ctor, calls [(first packet, packets)], and optionally slot / subset / async_join / env)"""
    c = {}
    for n in STREAMS:
        for p in packets_of(k):
            c["plain-n%d-p%d" % (n, p)] = dict(n=n, total=p, kind="speech", ctor={}, calls=[(0, p)])
    c["dtx-k%d" % k] = dict(n=33, total=30, kind="dtx", ctor=dict(dtx=1), calls=plan(k, 30))
    c["fs20-k%d" % k] = dict(n=33, total=2 * k + 3, kind="fs20", ctor=dict(framesize_ms=20), calls=[(0, 2 * k + 3)])
    c["wb-k%d" % k] = dict(n=33, total=2 * k + 3, kind="wb", ctor=dict(samplerate=32000, rate=24000), calls=[(0, 2 * k + 3)])
    # synthetic speech packets take 56 .. 114 bytes: some of every batch fit 80, some do not
    c["slot-k%d" % k] = dict(n=33, total=2 * k + 3, kind="speech", ctor={}, slot=80, calls=[(0, 2 * k + 3)])
    c["subset-k%d" % k] = dict(n=65, total=k + 1 + 2 * k + 3, kind="speech", ctor={}, calls=[(0, k + 1), (k + 1, 2 * k + 3)],
                               subset=[0] + list(range(3, 65, 2)) + [64])          # 33 rows in the second call
    c["async-k%d" % k] = dict(n=33, total=3 * k + 4, kind="speech", ctor={}, calls=[(0, 2 * k + 3), (2 * k + 3, k + 1)], async_join=True)
    c["group-k%d" % k] = dict(n=65, total=2 * k + 3, kind="speech", ctor={}, calls=[(0, 2 * k + 3)], env={"SOLO_ENC_GROUP": "32"})
    return c


def rows_of(case, call):
    """the streams a call encodes: every one, but the listed subset in the calls after the first"""
    return case["subset"] if case.get("subset") and call > 0 else list(range(case["n"]))


def run_case(torch, solo_amd, case):
    for key, v in case.get("env", {}).items():
        os.environ[key] = v
    try:
        slot = case.get("slot", 512)
        b = solo_amd.SoloBatch(case["n"], encoder=True, decoder=False, slot_bytes=slot, **case["ctor"])
        if case.get("async_join"):
            b.set_async_join(True)
        pcm = pcm_of(case["kind"], case["n"], case["total"])
        ins, outs = [], []
        for i, (p0, n) in enumerate(case["calls"]):
            rows = rows_of(case, i)
            ins.append(torch.from_numpy(np.ascontiguousarray(pcm[rows, p0:p0 + n])).to(b.device))
            outs.append((torch.full((len(rows), n, slot), FILL, dtype=torch.uint8, device=b.device),
                         torch.full((len(rows), n, 2), -7, dtype=torch.int16, device=b.device),
                         torch.full((len(rows),), -7, dtype=torch.int32, device=b.device)))
        torch.cuda.synchronize()
        for i, x in enumerate(ins):          # back to back: under async_join nothing orders two calls but the handle's own events
            b.encode(x, *outs[i], streams=rows_of(case, i) if case.get("subset") and i > 0 else None)
        if case.get("async_join"):
            b.wait_encode(1)
            b.wait_encode(0)
        torch.cuda.synchronize()
        return [tuple(t.cpu().numpy() for t in o) for o in outs]
    finally:
        for key in case.get("env", {}):
            os.environ.pop(key, None)


def main():
    knob, ks, out = sys.argv[1], [int(v) for v in sys.argv[2].split(",")], sys.argv[3]
    os.environ["SOLO_ENC_RC_BATCH"] = knob
    import torch
    import solo_amd
    res, done = {}, set()
    for k in ks:
        for name, case in cases(k).items():
            if name in done:
                continue
            done.add(name)
            for i, (bits, nb, st) in enumerate(run_case(torch, solo_amd, case)):
                res["%s/%d/bits" % (name, i)], res["%s/%d/nb" % (name, i)], res["%s/%d/st" % (name, i)] = bits, nb, st
    np.savez(out, **res)
    print("rc_batch_worker: knob %s, %d cases" % (knob, len(done)))


if __name__ == "__main__":
    main()
