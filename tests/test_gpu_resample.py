"""PCM resampler (solo_resample, solo_amd/csrc/solo_resample.h) on the GPU, byte for byte against the fixture recorded from the
compiled reference (tests/golden/resample.npz).  Where a shape goes beyond the fixture the rows are tiled fixture rows (row i = family
i % 6), so the expected data is still the fixture's; states are checked through what a further packet gives, with the independent model
of tests/resample_model.py continued from the fixture's state."""
import numpy as np
import pytest

import resample_lib as L
import resample_model as M
import solo_testlib as T

pytestmark = pytest.mark.gpu

R = 16                                                      # rows of a workgroup (SX_RS_ROWS)
pid = lambda p: "%d-%d" % (p[0] // 1000, p[1] // 1000)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(torch, t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def test_rows_per_group_is_what_the_shapes_assume():
    src = open(T.ROOT + "/solo_amd/csrc/solo_resample.h").read()
    assert "#define SX_RS_ROWS %d " % R in src


@pytest.mark.parametrize("pair", L.PAIRS, ids=pid)
def test_every_pair_equals_fixture(torch_cuda, pair):
    """6 rows x 4 packets in one call; then a packet of zeros, which must come out as the model gives it from the fixture's state"""
    import solo_amd
    torch = torch_cuda
    fs_in, fs_out = pair
    pcm, st = L.expected(fs_in, fs_out)
    x = L.inputs(fs_in)
    rs = solo_amd.Resampler(L.FAMILIES, fs_in, fs_out)
    assert rs.out_samples(x.shape[2]) == pcm.shape[2]
    out = host(torch, rs.run(dev(torch, x)))
    assert np.array_equal(out, pcm), np.argwhere(out != pcm)[:4]
    zeros = np.zeros((L.FAMILIES, 1, x.shape[2]), dtype=np.int16)
    tail = host(torch, rs.run(dev(torch, zeros)))
    want, _ = M.run_rows(fs_in, fs_out, zeros, st[:, -1])
    assert np.array_equal(tail, want)


@pytest.mark.parametrize("pair", ((48000, 16000), (16000, 48000), (16000, 32000)), ids=pid)
def test_four_calls_equal_one(torch_cuda, pair):
    import solo_amd
    torch = torch_cuda
    fs_in, fs_out = pair
    pcm, _ = L.expected(fs_in, fs_out)
    x = dev(torch, L.inputs(fs_in))
    rs = solo_amd.Resampler(L.FAMILIES, fs_in, fs_out)
    parts = [rs.run(x[:, p:p + 1].contiguous()) for p in range(L.PACKETS)]
    out = host(torch, torch.cat(parts, dim=1))
    assert np.array_equal(out, pcm)
    rs.reset()
    assert np.array_equal(host(torch, rs.run(x)), out)


@pytest.mark.parametrize("pair", L.PAIRS_20MS, ids=pid)
def test_20ms_packets_equal_fixture(torch_cuda, pair):
    import solo_amd
    torch = torch_cuda
    fs_in, fs_out = pair
    pcm, _ = L.expected(fs_in, fs_out, 20)
    rs = solo_amd.Resampler(L.FAMILIES, fs_in, fs_out)
    assert np.array_equal(host(torch, rs.run(dev(torch, L.inputs(fs_in, 20)))), pcm)


@pytest.mark.parametrize("n_rows", (1, R - 1, R + 1, 4 * R + 3))
@pytest.mark.parametrize("pair", ((48000, 32000), (32000, 48000)), ids=pid)
def test_row_counts_around_the_group_size(torch_cuda, pair, n_rows):
    import solo_amd
    torch = torch_cuda
    fs_in, fs_out = pair
    pcm, _ = L.expected(fs_in, fs_out)
    rs = solo_amd.Resampler(n_rows, fs_in, fs_out)
    guard = torch.full((n_rows + 1, L.PACKETS, pcm.shape[2]), 0x5A5A, dtype=torch.int16, device="cuda")
    out = rs.run(dev(torch, L.tiled(L.inputs(fs_in), n_rows)), out=guard[:n_rows])
    assert np.array_equal(host(torch, out), L.tiled(pcm, n_rows))
    assert bool((guard[n_rows] == 0x5A5A).all())


def test_listed_rows(torch_cuda):
    """every third row of 4R + 3: compact output, the unlisted rows' state untouched; two bad lists are refused and change nothing"""
    import solo_amd
    torch = torch_cuda
    fs_in, fs_out = 48000, 16000
    n = 4 * R + 3
    pcm = L.tiled(L.expected(fs_in, fs_out)[0], n)
    x = dev(torch, L.tiled(L.inputs(fs_in), n))
    rows = np.arange(0, n, 3)
    rest = np.setdiff1d(np.arange(n), rows)
    rs = solo_amd.Resampler(n, fs_in, fs_out)
    out, count = rs.run(x[rows, 0:1].contiguous(), rows=rows.tolist())
    assert rs.count(count) == {"rows": len(rows), "listed": len(rows)}
    assert np.array_equal(host(torch, out)[:, 0], pcm[rows, 0])
    # refused lists: not increasing, an index equal to n_rows
    for bad in ([3, 2, 7], [0, 5, n]):
        fill = torch.full((3, 1, pcm.shape[2]), 0x5A5A, dtype=torch.int16, device="cuda")
        o, c = rs.run(x[:3, 1:2].contiguous(), rows=torch.tensor(bad, dtype=torch.int32, device="cuda"), out=fill)
        assert rs.count(c)["rows"] == -1
        assert bool((o == 0x5A5A).all())
    # a full call of packet 0: the unlisted rows give packet 0's output (their state was never touched), the listed ones are one
    # packet ahead and give what the model makes of packet 0's samples after packet 0
    full = host(torch, rs.run(x[:, 0:1].contiguous()))
    assert np.array_equal(full[rest, 0], pcm[rest, 0])
    st0 = L.tiled(L.expected(fs_in, fs_out)[1], n)[:, 0]
    want, _ = M.run_rows(fs_in, fs_out, L.tiled(L.inputs(fs_in), n)[rows[:6], 0:1], st0[rows[:6]])
    assert np.array_equal(full[rows[:6]], want)


def test_reset_rows(torch_cuda):
    """after two packets rows 0 and 2 are reset: fed packet 0's samples again they give packet 0's output; the others go on"""
    import solo_amd
    torch = torch_cuda
    fs_in, fs_out = 16000, 48000
    pcm, st = L.expected(fs_in, fs_out)
    xin = L.inputs(fs_in)
    rs = solo_amd.Resampler(L.FAMILIES, fs_in, fs_out)
    assert np.array_equal(host(torch, rs.run(dev(torch, xin[:, :2]))), pcm[:, :2])
    rs.reset(rows=[0, 2])
    nxt = xin[:, 2:3].copy()
    nxt[[0, 2]] = xin[[0, 2], 0:1]
    out = host(torch, rs.run(dev(torch, nxt)))
    assert np.array_equal(out[[0, 2], 0], pcm[[0, 2], 0])
    assert np.array_equal(out[[1, 3, 4, 5], 0], pcm[[1, 3, 4, 5], 2])
    for bad in ([0, 0], [L.FAMILIES], [-1], []):
        with pytest.raises(ValueError):
            rs.reset(rows=bad)
    arr = np.array([1, 1], dtype=np.int32)
    assert rs.lib.solo_resample_reset_rows(rs.h, arr.ctypes.data, 2, None) == -1           # the library's own check of the host list
    assert rs.lib.solo_resample_reset_rows(rs.h, arr.ctypes.data, 0, None) == -1


def test_decoder_output_through_two_conversions(torch_cuda):
    """4 streams of the 16 kHz decoder goldens -> 16->32 -> 32->16: the layouts join without a repack (decode -> run -> mix / encode);
    expected = the model applied to the decoder's own PCM"""
    import solo_amd
    torch = torch_cuda
    z = np.load(T.GOLDEN + "/synth8x25.npz")
    n, P = 4, 3
    bits, nb = z["bits"][:n, :P], z["nbytes"][:n, :P]
    b = solo_amd.SoloBatch(n, encoder=True, decoder=True, slot_bytes=bits.shape[2])
    pcm, status = b.decode(dev(torch, bits), dev(torch, nb))
    up, down = solo_amd.Resampler(n, 16000, 32000), solo_amd.Resampler(n, 32000, 16000)
    wide = up.run(pcm)
    back = down.run(wide)
    b32 = solo_amd.SoloBatch(n, rate=15600, encoder=False, decoder=True, samplerate=32000)
    room = torch.zeros(n, dtype=torch.int32, device="cuda")
    mixed, _ = b32.mix(wide, room)                          # (accepted as it is: [n, P, 1280])
    _, _, est = b.encode(back)                              # (and so is [n, P, 640])
    torch.cuda.synchronize()
    assert int(status.abs().max()) == 0 and int(est.abs().max()) == 0 and tuple(mixed.shape) == (n, P, 1280)
    h = pcm.cpu().numpy()
    assert np.array_equal(h, z["dec_clean"][:n, :P])
    want_wide, _ = M.run_rows(16000, 32000, h)
    want_back, _ = M.run_rows(32000, 16000, want_wide)
    assert np.array_equal(wide.cpu().numpy(), want_wide)
    assert np.array_equal(back.cpu().numpy(), want_back)


def test_binding_argument_checks(torch_cuda):
    import solo_amd
    torch = torch_cuda
    for bad in ((16000, 16000), (48000, 8000), (44100, 16000), (16000, 96000)):
        with pytest.raises(ValueError):
            solo_amd.Resampler(4, *bad)
        assert not solo_amd.load_library().solo_resample_create(4, *bad)
    with pytest.raises(ValueError):
        solo_amd.Resampler(0, 16000, 32000)
    rs = solo_amd.Resampler(4, 16000, 32000)
    ok = torch.zeros((4, 2, 640), dtype=torch.int16, device="cuda")
    assert rs.check(ok) == (4, 2, 640, 1280)
    for bad in (ok.to(torch.int32), ok.float(), ok.cpu(), ok[:, :, ::2], ok.transpose(0, 1), ok[:, :, :639].contiguous(), ok[:, :, :100].contiguous(),
                ok[:3].contiguous(), ok[0]):
        with pytest.raises(ValueError):
            rs.run(bad)
    for bad_out in (torch.zeros((4, 2, 640), dtype=torch.int16, device="cuda"), torch.zeros((4, 1, 1280), dtype=torch.int16, device="cuda"),
                    torch.zeros((4, 2, 1280), dtype=torch.int32, device="cuda"), torch.zeros((4, 2, 2560), dtype=torch.int16, device="cuda")[:, :, ::2]):
        with pytest.raises(ValueError):
            rs.run(ok, out=bad_out)
    for bad_rows in ([1, 1], [2, 1], [0, 4], [-1, 0], []):
        with pytest.raises(ValueError):
            rs.run(ok[:2].contiguous(), rows=bad_rows)
    with pytest.raises(ValueError):
        rs.run(ok, rows=[0, 1])                             # two rows listed, four given
    with pytest.raises(ValueError):
        rs.out_samples(100)
    # the library's own refusals: nothing enqueued
    st = rs._stream()
    o = torch.zeros((4, 2, 1280), dtype=torch.int16, device="cuda")
    assert rs.lib.solo_resample(rs.h, ok.data_ptr(), 2, 100, o.data_ptr(), st) == -1
    assert rs.lib.solo_resample(rs.h, ok.data_ptr(), 0, 640, o.data_ptr(), st) == -1
    assert rs.lib.solo_resample(rs.h, None, 2, 640, o.data_ptr(), st) == -1
    assert rs.lib.solo_resample(rs.h, ok.data_ptr() + 2, 1, 640, o.data_ptr(), st) == -1
    assert rs.lib.solo_resample(rs.h, o.data_ptr(), 2, 640, o.data_ptr() + 16, st) == -1    # overlap
    c = torch.zeros(2, dtype=torch.int32, device="cuda")
    r4 = torch.arange(4, dtype=torch.int32, device="cuda")
    assert rs.lib.solo_resample_rows(rs.h, r4.data_ptr(), 5, ok.data_ptr(), 2, 640, o.data_ptr(), c.data_ptr(), st) == -1
    assert rs.lib.solo_resample_rows(rs.h, r4.data_ptr(), 0, ok.data_ptr(), 2, 640, o.data_ptr(), c.data_ptr(), st) == -1
    assert rs.lib.solo_resample_rows(rs.h, None, 4, ok.data_ptr(), 2, 640, o.data_ptr(), c.data_ptr(), st) == -1
    assert rs.lib.solo_resample_rows(rs.h, r4.data_ptr(), 4, ok.data_ptr(), 2, 640, o.data_ptr(), None, st) == -1
    assert rs.lib.solo_resample_out_samples(rs.h, 480) == 960 and rs.lib.solo_resample_out_samples(rs.h, 481) == -1
    torch.cuda.synchronize()
    assert not bool(o.any()) and not bool(c.any())
