"""The lifecycle that Resampler, Vad, Agc and Playout share (solo_rows of solo_amd/csrc/solo_api.hip, the kernels of solo_rows.h) at the two
corners the stages' own GPU tests do not reach: a listed reset of more rows than one list launch carries (SX_CTL_PER_LAUNCH = 128), and a
state round trip whose blob is not a whole number of 256-lane workgroups.  300 rows, one packet of the smallest size each stage takes."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 300
LISTED = list(range(299, 299 - 2 * 130, -2))                # 130 distinct rows, descending: two list launches, 128 + 2
OTHERS = np.setdiff1d(np.arange(N), LISTED)
PICK = [0, 3, 64, 127, 128, 200, 255, 298, 299]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def _pcm(torch, seed, samples):
    return torch.from_numpy(np.random.RandomState(seed).randint(-20000, 20000, (N, 1, samples)).astype(np.int16)).cuda()


def _host(torch, x):
    torch.cuda.synchronize()
    return x.cpu().numpy()


def _make(kind, packet_samples=8):
    import solo_amd
    if kind == "vad":
        return solo_amd.Vad(N, 160)
    if kind == "agc":
        return solo_amd.Agc(N)
    return solo_amd.Playout(N, packet_samples)


def _run_a_packet(torch, kind, o):
    """one packet through every row, so that no record is the initial one any more"""
    if kind == "vad":
        o.run(_pcm(torch, 11, 160))
    elif kind == "agc":
        o.run(_pcm(torch, 12, 256))
    else:
        # a plan on reports that start every row (2 packets ready, late counts that differ by row, no arrival: margin_min = depth), then a
        # held packet for every row: the second segment of the state
        rep = torch.zeros((N, 16), dtype=torch.int32, device="cuda")
        rep[:, 3], rep[:, 7], rep[:, 15] = 2, torch.arange(1, N + 1, dtype=torch.int32, device="cuda"), 8
        o.plan(rep, 8)
        blob = o.get_state()
        held = np.random.RandomState(13).randint(1, 256, (N, o.state_bytes - 128)).astype(np.uint8)
        blob[:, 128:] = torch.from_numpy(held).cuda()
        o.set_state(blob)


def _resampler_listed_reset(torch):
    """no state getter: the listed rows continue as a fresh object does, the others as an untouched twin"""
    import solo_amd
    o, twin, fresh = (solo_amd.Resampler(N, 16000, 8000) for _ in range(3))
    x0, x1 = _pcm(torch, 14, 160), _pcm(torch, 15, 160)
    o.run(x0)
    twin.run(x0)
    o.reset(rows=LISTED)
    y, y_twin, y_fresh = (_host(torch, r.run(x1)) for r in (o, twin, fresh))
    assert (y_twin != y_fresh).any(axis=(1, 2)).all()                           # the filter memory of every row is heard
    assert np.array_equal(y[LISTED], y_fresh[LISTED])
    assert np.array_equal(y[OTHERS], y_twin[OTHERS])


@pytest.mark.parametrize("kind", ["resample", "vad", "agc", "playout"])
def test_listed_reset_of_more_rows_than_a_list_launch(torch_cuda, kind):
    torch = torch_cuda
    if kind == "resample":
        return _resampler_listed_reset(torch)
    fresh = _host(torch, _make(kind).get_state())
    o = _make(kind)
    _run_a_packet(torch, kind, o)
    before = _host(torch, o.get_state())
    assert (before != fresh).any(axis=1).all()                                  # every record moved ...
    assert kind != "playout" or (before[:, 128:] != 0).all()                    # ... and every held packet is there
    o.reset(rows=LISTED)
    after = _host(torch, o.get_state())
    assert np.array_equal(after[LISTED], fresh[LISTED])
    assert np.array_equal(after[OTHERS], before[OTHERS])


@pytest.mark.parametrize("kind", ["vad", "agc", "playout"])
def test_state_round_trip_of_a_ragged_blob(torch_cuda, kind):
    """9 rows of 32, 16 and 32 + 160 words: 288, 144 and 1728 words, none a multiple of 256"""
    torch = torch_cuda
    fresh = _host(torch, _make(kind, 320).get_state())
    o = _make(kind, 320)
    assert (9 * o.state_bytes // 4) % 256 != 0
    _run_a_packet(torch, kind, o)
    before = _host(torch, o.get_state())
    blob = o.get_state(rows=PICK)
    assert np.array_equal(_host(torch, blob), before[PICK]) and (before[PICK] != fresh[PICK]).any(axis=1).all()
    o.reset()
    assert np.array_equal(_host(torch, o.get_state()), fresh)
    o.set_state(blob, rows=PICK)
    after = _host(torch, o.get_state())
    rest = np.setdiff1d(np.arange(N), PICK)
    assert np.array_equal(after[PICK], before[PICK])
    assert np.array_equal(after[rest], fresh[rest])
