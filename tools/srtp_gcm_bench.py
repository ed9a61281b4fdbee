#!/usr/bin/env python3
"""Cost of AEAD_AES_128_GCM next to AES-CM / HMAC-SHA1-80 in the SRTP and the SRTCP stage, in the protocol of tools/srtp_bench.py: 4096
streams x 1 packet (a tick: 8192 datagrams) and x 50, 13.6 kbps, levels on, every call through the C ABI with buffers allocated once.

  SRTP   the same packed datagrams (solo_rtp_pack with a trailer of 16, so that the wire is the same for all three) under three sessions
         of the same bindings: every stream keyed for AES-CM / HMAC-80 ("cm"), every stream for GCM ("gcm"), even streams GCM and odd
         ones AES-CM ("mixed").  solo_srtp_protect and solo_srtp_unprotect work in place, so every timed call is preceded by a device
         copy that puts the wire and the datagram table back; the copy is timed alone and taken off
  SRTCP  4096 packets of 88 bytes under a session keyed for HMAC and one keyed for GCM: solo_srtcp_protect of the same packets (restored
         likewise; the send indices advance with every call), and solo_srtcp_unprotect over windows of exactly BATCHES protected batches
         with rising indices, the receive records set back between the windows (a second look at a batch would be a replay, rejected
         in front of the tag); the copy into the working buffer is timed the same way and taken off

Every figure is ms per call: HIP events around back-to-back calls, the median over `runs` windows with the smallest and the largest next
to it.  Back-to-back calls measure the larger of the host's enqueue time and the device's time per call: the figures bound the call from
above.  The yardstick is the "cm" column of the same run.

  python tools/srtp_gcm_bench.py [--streams 4096] [--packets 1 50] [--runs 9] [--out profiles/srtp_gcm.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import solo_amd                       # noqa: E402
from solo_amd.synth import synth_stream  # noqa: E402
from rtp_bench import timed           # noqa: E402

TRAILER = solo_amd.SRTP_GCM_TAG_BYTES
BATCHES = 32
KERNELS = ("solo_srtp_protect_kernel", "solo_srtp_unprotect_kernel", "solo_srtcp_protect_kernel", "solo_srtcp_unprotect_kernel", "solo_srtp_gcm_protect_kernel",
           "solo_srtp_gcm_unprotect_kernel", "solo_srtcp_gcm_protect_kernel", "solo_srtcp_gcm_unprotect_kernel")


def less(r, copy):
    for k in ("ms", "min_ms", "max_ms"):
        r[k] = round(r[k] - copy["ms"], 5)
    r["restore_ms"] = copy["ms"]
    return r


def sessions(N, rng, seq_offset):
    """three sessions of the same bindings -> {name: (Rtp, tag of stream s)}"""
    ssrc, ts = [(i + 1) * 2654435761 % 2 ** 32 for i in range(N)], [int(v) for v in rng.integers(0, 2 ** 32, N)]
    roc = [(seq_offset[i] + 2 * 1000) >> 16 for i in range(N)]
    cm = rng.integers(0, 256, (N, solo_amd.SRTP_MASTER_BYTES), dtype=np.uint8)
    gcm = rng.integers(0, 256, (N, solo_amd.SRTP_GCM_MASTER_BYTES), dtype=np.uint8)
    out = {}
    for name, is_gcm in (("cm", lambda s: False), ("gcm", lambda s: True), ("mixed", lambda s: s % 2 == 0)):
        r = solo_amd.Rtp(N, 640)
        r.bind(list(range(N)), ssrc, ts, seq_offset, (96, 97), level_id=1)
        r.set_trailer(TRAILER)
        a, b = [s for s in range(N) if is_gcm(s)], [s for s in range(N) if not is_gcm(s)]
        if a:
            r.set_keys_gcm(a, tx=gcm[a], rx=gcm[a], rx_roc=[roc[s] for s in a])
        if b:
            r.set_keys(b, tx=cm[b], rx=cm[b], rx_roc=[roc[s] for s in b], tag_bytes=10)
        out[name] = (r, np.array([16 if is_gcm(s) else 10 for s in range(N)], np.int32))
    return out


def srtp_shape(torch, N, P, runs):
    pcm = torch.from_numpy(np.stack([synth_stream(i % 64, P) for i in range(N)]).reshape(N, P, 640)).cuda()
    tx = solo_amd.SoloBatch(N, rate=13600, encoder=True, decoder=False, slot_bytes=512)
    bits, nb, _ = tx.encode(pcm)
    records, payload, scount = tx.send_pack(bits, nb, first_seq=1000)
    sc = tx.send_count(scount)
    assert sc["records"] == sc["records_needed"] and sc["refused"] == 0
    n, M = sc["records"], records.shape[0]
    rng = np.random.default_rng(1)
    seq_offset = [int(v) for v in rng.integers(0, 2 ** 15, N)]
    ses = sessions(N, rng, seq_offset)
    level = torch.from_numpy(rng.integers(0, 128, (N, 64), dtype=np.uint8)).cuda()
    st, L = tx._stream(), tx.lib
    res = {"streams": N, "packets": P, "datagrams": n, "payload_bytes": sc["bytes"], "trailer": TRAILER}
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    cap = sc["bytes"] + (23 + TRAILER) * M
    dgrams, wire, cnt, scnt, out = z((M, 2), torch.int32), z((cap,), torch.uint8), z((8,), torch.int32), z((8,), torch.int32), z((M, 2), torch.int32)
    first = ses["cm"][0]
    res["rtp_pack"] = timed(torch, lambda: L.solo_rtp_pack(first.h, records.data_ptr(), scount.data_ptr(), M, payload.data_ptr(), payload.shape[0], level.data_ptr(), 64,
                                                           dgrams.data_ptr(), wire.data_ptr(), cap, cnt.data_ptr(), st), runs)
    c = first.pack_count(cnt)
    assert c["dgrams"] == c["dgrams_needed"] == n and c["refused"] == 0, c
    packed_dg, packed = dgrams.clone(), wire.clone()
    stream_of = records[:n, 0].cpu().numpy()

    def restore(dg_from, wire_from):
        def f():
            dgrams.copy_(dg_from)
            wire.copy_(wire_from)
            return 0
        return f
    put_packed = restore(packed_dg, packed)
    copy = timed(torch, put_packed, runs)
    for name, (rtp, tags) in ses.items():
        r = {}
        r["protect"] = less(timed(torch, lambda: put_packed() or L.solo_srtp_protect(rtp.h, records.data_ptr(), scount.data_ptr(), M, dgrams.data_ptr(), wire.data_ptr(), cap,
                                                                                     scnt.data_ptr(), st), runs), copy)
        pc = rtp.srtp_count(scnt)
        assert pc["ok"] == n and pc["no_key"] == 0 and pc["malformed"] == 0, pc
        prot_dg, prot = dgrams.clone(), wire.clone()
        grown = (prot_dg[:n, 1] - packed_dg[:n, 1]).cpu().numpy()
        assert np.array_equal(grown, tags[stream_of]), name
        put_prot = restore(prot_dg, prot)
        copy2 = timed(torch, put_prot, runs)
        r["unprotect"] = less(timed(torch, lambda: put_prot() or L.solo_srtp_unprotect(rtp.h, dgrams.data_ptr(), n, wire.data_ptr(), cap, out.data_ptr(), scnt.data_ptr(), st),
                                    runs), copy2)
        uc = rtp.srtp_count(scnt)
        assert uc["ok"] == n, uc
        assert bool((out[:n] == packed_dg[:n]).all())
        r["ns_per_datagram"] = {"protect": round(1e6 * r["protect"]["ms"] / n, 3), "unprotect": round(1e6 * r["unprotect"]["ms"] / n, 3)}
        res[name] = r
    for name in ("gcm", "mixed"):
        res[name]["over_cm"] = {k: round(res[name][k]["ms"] / res["cm"][k]["ms"], 3) for k in ("protect", "unprotect")}
    for rtp, _ in ses.values():
        rtp.close()
    tx.close()
    return res


def srtcp_shape(torch, N, runs):
    rng = np.random.default_rng(2)
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device="cuda")
    res = {"streams": N, "packet_bytes": 88, "batches": BATCHES}
    ssrc = [(i + 1) * 2246822519 % 2 ** 32 for i in range(N)]
    pkt = np.zeros((N, 112), np.uint8)                                 # 88 bytes of packet, room for either trailer, at a multiple of 4
    pkt[:, :88] = rng.integers(0, 256, (N, 88), dtype=np.uint8)
    pkt[:, 0], pkt[:, 1] = 0x80, 200
    pkt[:, 4:8] = np.array(ssrc, ">u4").view(np.uint8).reshape(N, 4)
    plain_w = torch.from_numpy(pkt.reshape(-1)).cuda()
    plain_d = torch.from_numpy(np.stack([112 * np.arange(N), np.full(N, 88)], 1).astype(np.int32)).cuda()
    idx, bcnt = torch.arange(N, dtype=torch.int32, device="cuda"), z((8,), torch.int32)
    bcnt[0] = N
    for name, trailer in (("cm", solo_amd.SRTCP_TRAILER_BYTES), ("gcm", solo_amd.SRTCP_GCM_TRAILER_BYTES)):
        ses, rtcp = solo_amd.Rtp(N, 640), solo_amd.Rtcp(N)
        ses.bind(list(range(N)), ssrc, 0, 0, (96, 97))
        rtcp.set_trailer(trailer)
        master = rng.integers(0, 256, (N, 28 if name == "gcm" else 30), dtype=np.uint8)
        set_keys = ses.set_rtcp_keys_gcm if name == "gcm" else ses.set_rtcp_keys
        set_keys(range(N), tx=master, rx=master)
        st, L = ses._stream(), ses.lib
        dg, wire, scnt, out = z((N, 2), torch.int32), z((112 * N,), torch.uint8), z((8,), torch.int32), z((N, 2), torch.int32)

        def put():
            dg.copy_(plain_d)
            wire.copy_(plain_w)
            return 0

        def protect():
            return put() or L.solo_srtcp_protect(rtcp.h, ses.h, idx.data_ptr(), N, bcnt.data_ptr(), dg.data_ptr(), wire.data_ptr(), 112 * N, scnt.data_ptr(), st)
        r = {"protect": less(timed(torch, protect, runs), timed(torch, put, runs))}
        pc = ses.srtcp_count(scnt)
        assert pc["ok"] == N, pc
        set_keys(range(N), tx=master, tx_index=0)
        batches = []
        for _ in range(BATCHES):
            assert protect() == 0
            batches.append((dg.clone(), wire.clone()))

        def window(with_call):
            set_keys(range(N), rx=master, rx_index=-1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for d, w in batches:
                wire.copy_(w)
                if with_call:
                    L.solo_srtcp_unprotect(ses.h, d.data_ptr(), N, wire.data_ptr(), 112 * N, out.data_ptr(), scnt.data_ptr(), st)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / BATCHES
        window(True)
        uc = ses.srtcp_count(scnt)
        assert uc["ok"] == N, uc
        both, copy = [window(True) for _ in range(runs)], [window(False) for _ in range(runs)]
        c = float(np.median(copy))
        r["unprotect"] = {"ms": round(float(np.median(both)) - c, 5), "min_ms": round(min(both) - c, 5), "max_ms": round(max(both) - c, 5), "restore_ms": round(c, 5),
                          "iters": BATCHES}
        res[name] = r
        ses.close()
    res["gcm"]["over_cm"] = {k: round(res["gcm"][k]["ms"] / res["cm"][k]["ms"], 3) for k in ("protect", "unprotect")}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--packets", type=int, nargs="+", default=[1, 50])
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from kernel_resources import kernel_resources
    seen = kernel_resources(solo_amd.LIB_PATH)
    kernels = {frag: {k: r[k] for k in ("vgpr", "sgpr", "scratch", "lds")} for frag in KERNELS for name, r in seen.items() if frag in name}
    res = {"runs": a.runs, "kernel_source_hash": solo_amd.kernel_source_hash(), "shader_clock_mhz_before": solo_amd.shader_clock_mhz(), "kernels": kernels, "srtp": []}
    for P in a.packets:
        res["srtp"].append(srtp_shape(torch, a.streams, P, a.runs))
        print("srtp %d x %d done" % (a.streams, P), file=sys.stderr, flush=True)
    res["srtcp"] = srtcp_shape(torch, a.streams, a.runs)
    res["shader_clock_mhz_after"] = solo_amd.shader_clock_mhz()
    txt = json.dumps(res, indent=1)
    print(txt)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
