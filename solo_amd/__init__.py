"""solo_amd -- thin Python binding of libsolo_mi355x.so (the MI355X-native SOLO encode/decode path).

PyTorch is used only as plumbing: device memory (tensors), HIP streams and torch.distributed.
All codec arithmetic runs in the hand-written gfx950 kernels of solo_amd/csrc/; there is no CPU
fallback -- importing works everywhere (so the ABI can be inspected on a CPU-only box), but creating
a `SoloBatch` without the built library or without a GPU raises.

The C ABI bound here is declared in include/solo_mi355x.h (the six AGR_Sate_* entry points of the
reference's interface/AGR_JC1_SDK_API.h plus the batched device-pointer API).
"""
import ctypes as C
import operator
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SOLO_LIB_OVERRIDE") or os.path.join(_HERE, "libsolo_mi355x.so")

PACKET_SAMPLES = 640
DEFAULT_SLOT_BYTES = 512

ABI_SYMBOLS = [
    "AGR_Sate_Encoder_Init", "AGR_Sate_Encoder_Encode", "AGR_Sate_Encoder_Uninit",
    "AGR_Sate_Decoder_Init", "AGR_Sate_Decoder_Decode", "AGR_Sate_Decoder_Uninit",
    "solo_batch_create", "solo_batch_destroy", "solo_batch_reset", "solo_batch_encode", "solo_batch_decode",
    "solo_batch_n_streams", "solo_batch_slot_bytes", "solo_kernel_name", "solo_version", "solo_batch_set_timing",
    "solo_batch_last_kernel_ms", "solo_batch_last_encode_chunks", "solo_batch_decode_split", "solo_batch_set_async_join",
    "solo_batch_wait_encode", "solo_debug_l0", "solo_debug_sum_sqr_shift", "solo_debug_rowops", "solo_debug_clock", "solo_debug_nsq",
    "solo_debug_waveops", "solo_debug_fn", "solo_debug_nsq_ex", "solo_debug_analysis", "solo_debug_coding", "solo_debug_dec_extract", "solo_debug_dec_synth",
    "solo_recv_create", "solo_recv_insert", "solo_recv_decode", "solo_recv_stats",
    "solo_batch_reset_streams", "solo_recv_reset_streams", "solo_batch_update_streams",
    "solo_batch_encode_streams", "solo_batch_decode_streams", "solo_recv_decode_streams",
    "solo_send_pack", "solo_send_pack_streams", "solo_mix", "solo_recv_track", "solo_recv_report",
    "solo_batch_state_bytes", "solo_batch_export_streams", "solo_batch_import_streams",
    "solo_resample_create", "solo_resample_destroy", "solo_resample_out_samples", "solo_resample_reset", "solo_resample_reset_rows",
    "solo_resample", "solo_resample_rows",
    "solo_mix_shared", "solo_send_fanout", "solo_mix_selected",
    "solo_timescale",
    "solo_vad_create", "solo_vad_destroy", "solo_vad_reset", "solo_vad_reset_rows", "solo_vad_get_state", "solo_vad_set_state",
    "solo_vad", "solo_vad_select",
    "solo_playout_create", "solo_playout_destroy", "solo_playout_reset", "solo_playout_reset_rows", "solo_playout_get_state",
    "solo_playout_set_state", "solo_playout_plan", "solo_playout_gather", "solo_playout_render", "solo_playout_tick",
    "solo_agc_create", "solo_agc_destroy", "solo_agc_reset", "solo_agc_reset_rows", "solo_agc_get_state", "solo_agc_set_state", "solo_agc",
    "solo_rtp_create", "solo_rtp_destroy", "solo_rtp_bind", "solo_rtp_unbind", "solo_rtp_pack", "solo_rtp_parse",
    "solo_rtp_set_trailer", "solo_srtp_set_keys", "solo_srtp_clear_keys", "solo_srtp_get_rx_index", "solo_srtp_protect", "solo_srtp_unprotect",
    "solo_srtp_set_keys_gcm", "solo_srtcp_set_keys_gcm",
    "solo_forward_create", "solo_forward_destroy", "solo_forward_reset", "solo_forward_reset_rooms", "solo_forward_get_state",
    "solo_forward_set_state", "solo_forward_levels", "solo_forward_route",
    "solo_rtcp_create", "solo_rtcp_destroy", "solo_rtcp_reset", "solo_rtcp_reset_rows", "solo_rtcp_get_state", "solo_rtcp_set_state",
    "solo_rtcp_set_cname", "solo_rtcp_received", "solo_rtcp_sent", "solo_rtcp_build", "solo_rtcp_parse",
    "solo_rtcp_set_trailer", "solo_srtcp_set_keys", "solo_srtcp_clear_keys", "solo_srtcp_get_index", "solo_srtcp_protect", "solo_srtcp_unprotect",
    "solo_batch_update_rates", "solo_rate_create", "solo_rate_destroy", "solo_rate_reset", "solo_rate_reset_rows", "solo_rate_get_state",
    "solo_rate_set_state", "solo_rate_update", "solo_rate_send_mask",
]


class USER_Ctrl_enc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "mode", "targetRate_bps", "samplerate", "dtx_enable", "framesize_ms",
        "joint_enable", "joint_mode", "useMDIndex")]


class USER_Ctrl_dec(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "packetLoss_perc", "samplerate", "framesize_ms", "joint_enable", "joint_mode", "useMDIndex")]


class solo_send_count_t(C.Structure):
    """what a solo_send_pack call wrote and what it needed (include/solo_mi355x.h); 32 bytes"""
    _fields_ = [("records", C.c_int32), ("records_needed", C.c_int32), ("bytes", C.c_int64), ("bytes_needed", C.c_int64),
                ("empty", C.c_int32), ("refused", C.c_int32)]


class solo_mix_count_t(C.Structure):
    """what a solo_mix call did (include/solo_mi355x.h); 16 bytes"""
    _fields_ = [("rows", C.c_int32), ("rooms", C.c_int32), ("clipped", C.c_int64)]


class solo_mix_shared_count_t(C.Structure):
    """what a solo_mix_shared call did (include/solo_mi355x.h); 24 bytes"""
    _fields_ = [("rows", C.c_int32), ("rooms", C.c_int32), ("speakers", C.c_int32), ("shared", C.c_int32), ("clipped", C.c_int64)]


class solo_mix_selected_count_t(C.Structure):
    """what a solo_mix_selected call did (include/solo_mi355x.h); 32 bytes"""
    _fields_ = [("rows", C.c_int32), ("rooms", C.c_int32), ("speakers", C.c_int32), ("shared", C.c_int32), ("clipped", C.c_int64),
                ("selected", C.c_int32), ("silent", C.c_int32)]


class solo_timescale_count_t(C.Structure):
    """what a solo_timescale call did (include/solo_mi355x.h); 16 bytes"""
    _fields_ = [("rows", C.c_int32), ("blocks", C.c_int32), ("cost", C.c_int64)]


class solo_resample_count_t(C.Structure):
    """what a solo_resample_rows call did (include/solo_mi355x.h); 8 bytes"""
    _fields_ = [("rows", C.c_int32), ("listed", C.c_int32)]


class solo_vad_count_t(C.Structure):
    """what a solo_vad / solo_vad_select call did (include/solo_mi355x.h); 16 bytes; rows = -1: refused on the device"""
    _fields_ = [("rows", C.c_int32), ("rooms", C.c_int32), ("selected", C.c_int32), ("changes", C.c_int32)]


class solo_vad_select_params_t(C.Structure):
    """the policy of a solo_vad_select call (include/solo_mi355x.h); 20 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("max_speakers", "on_q8", "off_q8", "hang_packets", "stick")]


class solo_agc_params_t(C.Structure):
    """the policy of a solo_agc call (include/solo_mi355x.h); 40 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("target_level", "max_boost_db", "max_cut_db", "sa_on_q8", "gate_level", "alpha_q8", "slew_up_q8", "slew_down_q8",
                                         "ceiling", "release_q15")]


class solo_agc_count_t(C.Structure):
    """what a solo_agc call did (include/solo_mi355x.h); 16 bytes; rows = -1: list refused on the device"""
    _fields_ = [(n, C.c_int32) for n in ("rows", "speech", "limited", "zero")]


class solo_playout_params_t(C.Structure):
    """the policy of a solo_playout_plan / _render / _tick call (include/solo_mi355x.h); 32 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("start_ready", "max_span", "window", "tolerate", "lo", "hi", "cooldown", "cost_gate")]


class solo_playout_plan_count_t(C.Structure):
    """what a solo_playout_plan call decided (include/solo_mi355x.h); 16 bytes; n_one = -1: list refused on the device"""
    _fields_ = [(n, C.c_int32) for n in ("n_one", "n_two", "n_stretch", "listed")]


class solo_playout_render_count_t(C.Structure):
    """rows per outcome of a solo_playout_render call (include/solo_mi355x.h); 32 bytes; idle = -1: list refused on the device"""
    _fields_ = [(n, C.c_int32) for n in ("idle", "normal", "held", "stretch", "stretch_gated", "accel", "accel_gated", "accel_forced")]


class solo_playout_count_t(C.Structure):
    """what a solo_playout_tick call did: the plan's count, then the render's; 48 bytes"""
    _fields_ = [("plan", solo_playout_plan_count_t), ("render", solo_playout_render_count_t)]


class solo_migrate_count_t(C.Structure):
    """what a solo_batch_export_streams / solo_batch_import_streams call did (include/solo_mi355x.h); 16 bytes"""
    _fields_ = [("streams", C.c_int32), ("refused", C.c_int32), ("bytes", C.c_int64)]


class solo_recv_report_t(C.Structure):
    """one stream's queue and counters as solo_recv_report writes them (include/solo_mi355x.h); 64 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("play", "queued", "complete", "ready", "span", "head")] + \
               [(n, C.c_uint32) for n in ("inserted", "late", "ahead", "duplicate", "bad", "played_both", "played_md1", "played_md2", "played_none")] + \
               [("margin_min", C.c_int32)]


class solo_recv_report_count_t(C.Structure):
    """how many rows a solo_recv_report call selected, of how many listed; 8 bytes; selected = -1: list refused on the device"""
    _fields_ = [("selected", C.c_int32), ("listed", C.c_int32)]


class solo_dgram_t(C.Structure):
    """one datagram inside a wire buffer (include/solo_mi355x.h); 8 bytes"""
    _fields_ = [("offset", C.c_int32), ("len", C.c_int32)]


class solo_rtp_pack_count_t(C.Structure):
    """what a solo_rtp_pack call wrote and what it needed (include/solo_mi355x.h); 32 bytes; dgrams = -1: the list behind the records was refused"""
    _fields_ = [("dgrams", C.c_int32), ("dgrams_needed", C.c_int32), ("bytes", C.c_int64), ("bytes_needed", C.c_int64),
                ("refused", C.c_int32), ("reserved", C.c_int32)]


class solo_rtp_parse_count_t(C.Structure):
    """datagrams per verdict of a solo_rtp_parse call (include/solo_mi355x.h); 32 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("accepted", "with_level", "malformed", "version", "unknown_ssrc", "unknown_pt", "timestamp", "reserved")]


class solo_srtp_count_t(C.Structure):
    """datagrams per verdict of a solo_srtp_protect / solo_srtp_unprotect call (include/solo_mi355x.h); 32 bytes; ok = -1: the list behind
    protect's records was refused"""
    _fields_ = [(n, C.c_int32) for n in ("ok", "skipped", "malformed", "unknown_ssrc", "no_key", "auth_failed", "reserved0", "reserved1")]


class solo_srtcp_count_t(C.Structure):
    """datagrams per verdict of a solo_srtcp_protect / solo_srtcp_unprotect call (include/solo_mi355x.h); 32 bytes; ok = -1: the list
    behind protect's datagrams was refused"""
    _fields_ = [(n, C.c_int32) for n in ("ok", "skipped", "malformed", "unknown_ssrc", "no_key", "auth_failed", "replayed", "exhausted")]


class solo_rtcp_received_count_t(C.Structure):
    """datagrams per outcome of a solo_rtcp_received call (include/solo_mi355x.h); 32 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("counted", "first", "in_order", "misordered", "dropout_pending", "resynced", "not_counted", "reserved")]


class solo_rtcp_sent_count_t(C.Structure):
    """records of a solo_rtcp_sent call; 32 bytes; sent = -1: the records were refused"""
    _fields_ = [(n, C.c_int32) for n in ("sent", "skipped") + tuple("reserved%d" % k for k in range(6))]


class solo_rtcp_build_count_t(C.Structure):
    """packets and bytes of a solo_rtcp_build call, written and needed; 32 bytes; built = -1: the list was refused on the device"""
    _fields_ = [("built", C.c_int32), ("built_needed", C.c_int32), ("bytes", C.c_int64), ("bytes_needed", C.c_int64), ("refused", C.c_int32),
                ("with_sr", C.c_int32)]


class solo_rtcp_parse_count_t(C.Structure):
    """datagrams per verdict of a solo_rtcp_parse call, then what the accepted ones held; 64 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("accepted", "malformed", "version", "first_type", "length", "sr", "blocks", "unknown_ssrc", "bye",
                                         "skipped") + tuple("reserved%d" % k for k in range(6))]


class solo_rtcp_feedback_t(C.Structure):
    """what a peer's report block says about one of our streams (solo_rtcp_parse); 32 bytes"""
    _fields_ = [("seen", C.c_int32), ("fraction_lost", C.c_int32), ("cum_lost", C.c_int32), ("ext_high_seq", C.c_uint32), ("jitter", C.c_uint32),
                ("lsr", C.c_uint32), ("dlsr", C.c_uint32), ("rtt", C.c_int32)]


class solo_rate_apply_count_t(C.Structure):
    """what a solo_batch_update_rates call did (include/solo_mi355x.h); 16 bytes; applied = -1: list refused on the device"""
    _fields_ = [(n, C.c_int32) for n in ("applied", "kept", "refused", "listed")]


class solo_rate_params_t(C.Structure):
    """the policy of a solo_rate_update call (include/solo_mi355x.h); 48 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("min_bps", "max_bps", "start_bps", "quantum_bps", "lo_q8", "hi_q8", "inc_q8", "rtt_guard", "stale_calls", "thin_after",
                                         "thin_release", "reserved")]


class solo_rate_count_t(C.Structure):
    """what a solo_rate_update call did (include/solo_mi355x.h); 64 bytes"""
    _fields_ = [(n, C.c_int32) for n in ("rows", "started", "used", "repeated", "increased", "decreased", "held", "delayed", "stale", "bye", "thin_on",
                                         "thin_off", "thin_rows", "changed", "reserved0", "reserved1")]


class solo_forward_row_t(C.Structure):
    """what solo_forward_levels gathers per row from the arrivals of a call (include/solo_mi355x.h); 16 bytes"""
    _fields_ = [("min_seq", C.c_int32), ("max_seq", C.c_int32), ("dgrams", C.c_int32), ("sa", C.c_uint8), ("level", C.c_uint8), ("byte", C.c_uint8),
                ("pad", C.c_uint8)]


class solo_forward_count_t(C.Structure):
    """arrivals per verdict of a solo_forward_route call and the slots that changed their source (include/solo_mi355x.h); 32 bytes;
    forwarded = -1: a room id was refused on the device"""
    _fields_ = [(n, C.c_int32) for n in ("forwarded", "rejected", "no_desc", "no_room", "not_selected", "no_slot", "stale", "switches")]


SRTP_MASTER_BYTES = 30
SRTCP_TRAILER_BYTES = 14
SRTP_GCM_MASTER_BYTES = 28      # AEAD_AES_128_GCM (RFC 7714): master key (16) || master salt (12)
SRTP_GCM_TAG_BYTES = 16
SRTCP_GCM_TRAILER_BYTES = 20    # the tag, then the E || index word
RECV_REPORT_CLEAR_MARGIN = 1

_lib = None


def kernel_source_hash():
    """sha256 (first 16 hex digits) over the kernel sources solo_amd/csrc/* in name order: identifies the BUILD a benchmark line or a
    profile summary belongs to (the GPU box has no .git; profiles/*.json carry the same field, bench.py compares them).  Build
    flags from solo_amd/build_flags.txt count as source."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(_HERE, "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".h", ".hip", ".inc")):
            h.update(f.encode())
            h.update(open(os.path.join(d, f), "rb").read())
    flags = build_flags()
    if flags:                       # (an empty / absent flags file leaves the hash of the sources alone)
        h.update(" ".join(flags).encode())
    return h.hexdigest()[:16]


def build_flags():
    """Extra -D options the library is built with (solo_amd/build_flags.txt, one per line, '#' comments): part of a build's identity
    together with the sources, so that a profile taken from a flag variant is attributed to it (__graft_entry__.build() reads the
    same file)."""
    p = os.path.join(_HERE, "build_flags.txt")
    if not os.path.exists(p):
        return []
    return [l.strip() for l in open(p) if l.strip() and not l.strip().startswith("#")]


def load_library():
    """Loads libsolo_mi355x.so (raises if it has not been built: see __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libsolo_mi355x.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'`; "
                           "this package has no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.solo_batch_create.restype = C.c_void_p
    lib.solo_batch_create.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32]
    lib.solo_batch_destroy.argtypes = [C.c_void_p]
    lib.solo_batch_reset.argtypes = [C.c_void_p, C.c_void_p]
    lib.solo_batch_reset.restype = C.c_int32
    lib.solo_batch_reset_streams.restype = C.c_int32
    lib.solo_batch_reset_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_batch_update_streams.restype = C.c_int32
    lib.solo_batch_update_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_recv_reset_streams.restype = C.c_int32
    lib.solo_recv_reset_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.solo_batch_encode.restype = C.c_int32
    lib.solo_batch_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_batch_encode_streams.restype = C.c_int32
    lib.solo_batch_encode_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_batch_decode_streams.restype = C.c_int32
    lib.solo_batch_decode_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                              C.c_void_p]
    lib.solo_recv_decode_streams.restype = C.c_int32
    lib.solo_recv_decode_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_batch_decode.restype = C.c_int32
    lib.solo_batch_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_batch_n_streams.argtypes = [C.c_void_p]
    lib.solo_batch_slot_bytes.argtypes = [C.c_void_p]
    lib.solo_batch_set_timing.restype = C.c_int32
    lib.solo_batch_set_timing.argtypes = [C.c_void_p, C.c_int32]
    lib.solo_batch_last_kernel_ms.restype = C.c_int32
    lib.solo_batch_last_kernel_ms.argtypes = [C.c_void_p, C.c_void_p]
    lib.solo_batch_decode_split.restype = C.c_int32
    lib.solo_batch_decode_split.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                            C.c_void_p, C.c_void_p]
    lib.solo_recv_create.restype = C.c_int32
    lib.solo_recv_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.solo_recv_insert.restype = C.c_int32
    lib.solo_recv_insert.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    lib.solo_recv_decode.restype = C.c_int32
    lib.solo_recv_decode.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_recv_stats.restype = C.c_int32
    lib.solo_recv_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_recv_track.restype = C.c_int32
    lib.solo_recv_track.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
    lib.solo_recv_report.restype = C.c_int32
    lib.solo_recv_report.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p]
    _send = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.solo_send_pack.restype = C.c_int32
    lib.solo_send_pack.argtypes = [C.c_void_p] + _send
    lib.solo_send_pack_streams.restype = C.c_int32
    lib.solo_send_pack_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_int32] + _send
    lib.solo_mix.restype = C.c_int32
    lib.solo_mix.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_void_p]
    lib.solo_mix_shared.restype = C.c_int32
    lib.solo_mix_shared.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 12
    lib.solo_mix_selected.restype = C.c_int32
    lib.solo_mix_selected.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32] + [C.c_void_p] * 14
    lib.solo_timescale.restype = C.c_int32
    lib.solo_timescale.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_send_fanout.restype = C.c_int32
    lib.solo_send_fanout.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32] + _send[2:]
    lib.solo_batch_state_bytes.restype = C.c_int64
    lib.solo_batch_state_bytes.argtypes = [C.c_void_p, C.c_int32]
    for f in (lib.solo_batch_export_streams, lib.solo_batch_import_streams):
        f.restype = C.c_int32
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    # the row-state objects: their create calls differ (the table), their lifecycle calls do not
    for prefix, create_args, has_state in (("resample", 3, False), ("vad", 2, True), ("playout", 2, True), ("agc", 1, True)):
        sigs = {"create": (C.c_void_p, [C.c_int32] * create_args), "destroy": (None, [C.c_void_p]), "reset": (C.c_int32, [C.c_void_p, C.c_void_p]),
                "reset_rows": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p])}
        if has_state:
            sigs["get_state"] = sigs["set_state"] = (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])
        for name, (restype, argtypes) in sigs.items():
            f = getattr(lib, "solo_%s_%s" % (prefix, name))
            f.restype, f.argtypes = restype, list(argtypes)
    lib.solo_resample_out_samples.restype = C.c_int32
    lib.solo_resample_out_samples.argtypes = [C.c_void_p, C.c_int32]
    lib.solo_resample.restype = C.c_int32
    lib.solo_resample.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    lib.solo_vad.restype = C.c_int32
    lib.solo_vad.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_vad_select.restype = C.c_int32
    lib.solo_vad_select.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                    C.POINTER(solo_vad_select_params_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _pp = C.POINTER(solo_playout_params_t)
    lib.solo_playout_plan.restype = C.c_int32
    lib.solo_playout_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, _pp] + [C.c_void_p] * 6
    lib.solo_playout_gather.restype = C.c_int32
    lib.solo_playout_gather.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.solo_playout_render.restype = C.c_int32
    lib.solo_playout_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, _pp, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32] + [C.c_void_p] * 13
    lib.solo_playout_tick.restype = C.c_int32
    lib.solo_playout_tick.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _pp] + [C.c_void_p] * 5
    lib.solo_agc.restype = C.c_int32
    lib.solo_agc.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                             C.POINTER(solo_agc_params_t), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_rtp_create.restype = C.c_void_p
    lib.solo_rtp_create.argtypes = [C.c_int32, C.c_int32]
    lib.solo_rtp_destroy.restype = None
    lib.solo_rtp_destroy.argtypes = [C.c_void_p]
    lib.solo_rtp_bind.restype = C.c_int32
    lib.solo_rtp_bind.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.solo_rtp_unbind.restype = C.c_int32
    lib.solo_rtp_unbind.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.solo_rtp_pack.restype = C.c_int32
    lib.solo_rtp_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_void_p, C.c_void_p]
    lib.solo_rtp_parse.restype = C.c_int32
    lib.solo_rtp_parse.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_rtp_set_trailer.restype = C.c_int32
    lib.solo_rtp_set_trailer.argtypes = [C.c_void_p, C.c_int32]
    lib.solo_srtp_set_keys.restype = C.c_int32
    lib.solo_srtp_set_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.solo_srtp_set_keys_gcm.restype = C.c_int32
    lib.solo_srtp_set_keys_gcm.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_srtcp_set_keys_gcm.restype = C.c_int32
    lib.solo_srtcp_set_keys_gcm.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_srtp_clear_keys.restype = C.c_int32
    lib.solo_srtp_clear_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.solo_srtp_get_rx_index.restype = C.c_int32
    lib.solo_srtp_get_rx_index.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.solo_srtp_protect.restype = C.c_int32
    lib.solo_srtp_protect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.solo_srtp_unprotect.restype = C.c_int32
    lib.solo_srtp_unprotect.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    for name, (restype, argtypes) in {"create": (C.c_void_p, [C.c_int32, C.c_int32]), "destroy": (None, [C.c_void_p]), "reset": (C.c_int32, [C.c_void_p, C.c_void_p]),
                                      "reset_rooms": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
                                      "get_state": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
                                      "set_state": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p])}.items():
        f = getattr(lib, "solo_forward_" + name)
        f.restype, f.argtypes = restype, argtypes
    lib.solo_forward_levels.restype = C.c_int32
    lib.solo_forward_levels.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_forward_route.restype = C.c_int32
    lib.solo_forward_route.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for name, (restype, argtypes) in {"create": (C.c_void_p, [C.c_int32]), "destroy": (None, [C.c_void_p]), "reset": (C.c_int32, [C.c_void_p, C.c_void_p]),
                                      "reset_rows": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
                                      "get_state": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
                                      "set_state": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
                                      "set_cname": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
                                      "received": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32, C.c_void_p,
                                                               C.c_void_p]),
                                      "sent": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
                                      "build": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p,
                                                            C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
                                      "parse": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_uint64,
                                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p])}.items():
        f = getattr(lib, "solo_rtcp_" + name)
        f.restype, f.argtypes = restype, argtypes
    for name, (restype, argtypes) in {"create": (C.c_void_p, [C.c_int32]), "destroy": (None, [C.c_void_p]), "reset": (C.c_int32, [C.c_void_p, C.c_void_p]),
                                      "reset_rows": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
                                      "get_state": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
                                      "set_state": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
                                      "update": (C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
                                      "send_mask": (C.c_int32, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                                                C.c_void_p, C.c_void_p])}.items():
        f = getattr(lib, "solo_rate_" + name)
        f.restype, f.argtypes = restype, argtypes
    lib.solo_batch_update_rates.restype = C.c_int32
    lib.solo_batch_update_rates.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_rtcp_set_trailer.restype = C.c_int32
    lib.solo_rtcp_set_trailer.argtypes = [C.c_void_p, C.c_int32]
    lib.solo_srtcp_set_keys.restype = C.c_int32
    lib.solo_srtcp_set_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_srtcp_clear_keys.restype = C.c_int32
    lib.solo_srtcp_clear_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.solo_srtcp_get_index.restype = C.c_int32
    lib.solo_srtcp_get_index.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_srtcp_protect.restype = C.c_int32
    lib.solo_srtcp_protect.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.solo_srtcp_unprotect.restype = C.c_int32
    lib.solo_srtcp_unprotect.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_resample_rows.restype = C.c_int32
    lib.solo_resample_rows.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_batch_set_async_join.restype = C.c_int32
    lib.solo_batch_set_async_join.argtypes = [C.c_void_p, C.c_int32]
    lib.solo_batch_wait_encode.restype = C.c_int32
    lib.solo_batch_wait_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
    lib.solo_batch_last_encode_chunks.restype = C.c_int32
    lib.solo_batch_last_encode_chunks.argtypes = [C.c_void_p]
    lib.solo_debug_rowops.restype = C.c_int32
    lib.solo_debug_rowops.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_debug_waveops.restype = C.c_int32
    lib.solo_debug_waveops.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_debug_fn.restype = C.c_int32
    lib.solo_debug_fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]
    lib.solo_debug_nsq.restype = C.c_int32
    lib.solo_debug_nsq.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    # stage probes of the encoder: (samplerate, silk_rate_bps, useMDIndex, joint, dtx, frames_per_packet, n_streams, n_packets, ...)
    lib.solo_debug_nsq_ex.restype = C.c_int32
    lib.solo_debug_nsq_ex.argtypes = [C.c_int32] * 8 + [C.c_void_p, C.c_void_p]
    lib.solo_debug_analysis.restype = C.c_int32
    lib.solo_debug_analysis.argtypes = [C.c_int32] * 9 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_debug_coding.restype = C.c_int32
    lib.solo_debug_coding.argtypes = [C.c_int32] * 10 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.solo_debug_dec_extract.restype = C.c_int32
    lib.solo_debug_dec_extract.argtypes = [C.c_int32] * 8 + [C.c_void_p] * 5
    lib.solo_debug_dec_synth.restype = C.c_int32
    lib.solo_debug_dec_synth.argtypes = [C.c_int32] * 8 + [C.c_void_p] * 7 + [C.c_int32]
    lib.solo_debug_clock.restype = C.c_int32
    lib.solo_debug_clock.argtypes = [C.c_void_p]
    lib.solo_kernel_name.restype = C.c_char_p
    lib.solo_kernel_name.argtypes = [C.c_int32]
    lib.solo_version.restype = C.c_char_p
    lib.AGR_Sate_Encoder_Init.restype = C.c_void_p
    lib.AGR_Sate_Encoder_Init.argtypes = [C.c_void_p]
    lib.AGR_Sate_Encoder_Encode.restype = C.c_int32
    lib.AGR_Sate_Encoder_Encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    lib.AGR_Sate_Encoder_Uninit.argtypes = [C.c_void_p]
    lib.AGR_Sate_Decoder_Init.restype = C.c_void_p
    lib.AGR_Sate_Decoder_Init.argtypes = [C.c_void_p]
    lib.AGR_Sate_Decoder_Decode.restype = C.c_int32
    lib.AGR_Sate_Decoder_Decode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32]
    lib.AGR_Sate_Decoder_Uninit.argtypes = [C.c_void_p]
    _lib = lib
    return lib


def shader_clock_mhz():
    """Effective shader clock (MHz) while every SIMD of the current device runs vector instructions for ~1 ms (solo_debug_clock)."""
    v = C.c_double(0.0)
    if load_library().solo_debug_clock(C.byref(v)) != 0:
        return None
    return float(v.value)


def default_enc_ctrl(rate=13600, use_md_index=0, joint=0, dtx=0, samplerate=16000, framesize_ms=40):
    """Defaults of the reference CLI (JC1_SDK_SRC_ARM/test/enc_main.c:92-99); joint=1 is its `-joint 1`: one 40 ms high-band
    frame per packet (4 high-band bytes instead of 8)."""
    return USER_Ctrl_enc(mode=2, targetRate_bps=rate, samplerate=samplerate, dtx_enable=1 if dtx else 0, framesize_ms=framesize_ms,
                         joint_enable=1 if joint else 0, joint_mode=1 if joint else 0, useMDIndex=use_md_index)


def default_dec_ctrl(use_md_index=0, joint=0, samplerate=16000, framesize_ms=40):
    return USER_Ctrl_dec(packetLoss_perc=0, samplerate=samplerate, framesize_ms=framesize_ms, joint_enable=1 if joint else 0,
                         joint_mode=1 if joint else 0, useMDIndex=use_md_index)


# ---- the argument checks every method below shares: a bad argument raises ValueError before anything reaches the library ----
def _tensor(name, x, dtype, shape, optional=False):
    """x must be a contiguous CUDA tensor of `dtype` whose shape is `shape` (None = that dimension is free), or None where `optional`
    -> its shape as a tuple (None for an absent optional).  Reads is_cuda, dtype, is_contiguous() and shape, nothing else, and
    does no work on the device."""
    if x is None and optional:
        return None
    if getattr(x, "is_cuda", False) and x.dtype == dtype and x.is_contiguous():
        got = tuple(x.shape)
        if len(got) == len(shape):
            for w, g in zip(shape, got):             # (a plain loop: this runs a dozen times in a one-packet call)
                if w is not None and w != g:
                    break
            else:
                return got
    raise ValueError("%s: a contiguous %s CUDA tensor [%s]%s" % (name, str(dtype).split(".")[-1], ", ".join("n" if w is None else str(w) for w in shape),
                                                                 " or None" if optional else ""))


def _ptr(x):
    return None if x is None else x.data_ptr()


def _counts(struct, count):
    """a count tensor as the dict of the fields of `struct` (synchronises)"""
    c = struct.from_buffer_copy(count.cpu().numpy().tobytes())
    return {k: int(getattr(c, k)) for k, _ in struct._fields_}


def _host_list(rows):
    return [int(v) for v in (rows.tolist() if hasattr(rows, "tolist") else rows)]


def _increasing(name, rows, n):
    """a host sequence of indices inside [0, n), strictly increasing -> list"""
    idx = _host_list(rows)
    if not idx or any(b <= a for a, b in zip(idx, idx[1:])) or idx[0] < 0 or idx[-1] >= n:
        raise ValueError("%s: strictly increasing indices inside [0, %d)" % (name, n))
    return idx


def _distinct(name, rows, n):
    """a host sequence of indices inside [0, n), none twice -> list"""
    idx = _host_list(rows)
    if not 0 < len(idx) <= n or any(v < 0 or v >= n for v in idx) or len(set(idx)) != len(idx):
        raise ValueError("%s: 1 .. %d indices inside [0, %d), none twice" % (name, n, n))
    return idx


def debug_fn(samplerate, fn, records, out):
    """Function-level probe of the encoder's LPC / NLSF stage functions (solo_debug_fn, include/solo_mi355x.h; the functions and their
    records: solo_amd/csrc/solo_fn_probe.h): one call of stage function `fn` per row of `records` (int32 [n_cases, in_words]) into the
    same row of `out` (int32 [n_cases, out_words]), in the build of `samplerate`; runs on the current stream and waits for it.  -> out"""
    import torch
    n, _ = _tensor("records", records, torch.int32, (None, None))
    _tensor("out", out, torch.int32, (n, None))
    r = load_library().solo_debug_fn(int(samplerate), int(fn), n, _ptr(records), records.shape[1], _ptr(out), out.shape[1],
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream))
    if r:
        raise ValueError("solo_debug_fn -> %d (no such fn, or not its record sizes)" % r if r == -1 else "solo_debug_fn -> %d" % r)
    return out


class SoloBatch:
    """N independent SOLO streams on the current HIP device (one wavefront per stream)."""

    def __init__(self, n_streams, rate=13600, encoder=True, decoder=True, slot_bytes=DEFAULT_SLOT_BYTES, use_md_index=0, joint=0, dtx=0,
                 samplerate=16000, framesize_ms=40):
        """samplerate = 32000: the 32 kHz mode of the reference (`-Fs_API 32000`: 1280-sample packets, SILK wide band; rate >= 15600).
        framesize_ms = 20 (`-framesize 20`, AGR_BWE_SDK_API.c:100-115): packets of ONE 20 ms SILK frame + one 4-byte high-band frame, half as
        many samples per packet; not with joint=1 (its high-band frame is 40 ms)."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("solo_amd needs a HIP device (MI355X); there is no CPU path")
        self.torch = torch
        self.lib = load_library()
        self.n_streams = int(n_streams)
        self.slot = int(slot_bytes)
        if framesize_ms not in (20, 40):
            raise ValueError("framesize_ms must be 40 or 20")
        self._enc = default_enc_ctrl(rate, use_md_index, joint, dtx, samplerate, framesize_ms) if encoder else None
        if samplerate not in (16000, 32000):
            raise ValueError("samplerate must be 16000 or 32000")
        self.packet_samples = PACKET_SAMPLES * samplerate // 16000 * framesize_ms // 40
        self.samplerate = samplerate
        self._dec = default_dec_ctrl(use_md_index, joint, samplerate, framesize_ms) if decoder else None
        self.h = self.lib.solo_batch_create(self.n_streams, C.byref(self._enc) if encoder else None,
                                            C.byref(self._dec) if decoder else None, self.slot)
        if not self.h:
            raise RuntimeError("solo_batch_create failed (unsupported configuration, no GPU, or out of memory)")
        self.device = torch.device("cuda", torch.cuda.current_device())

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def reset(self):
        r = self.lib.solo_batch_reset(self.h, self._stream())
        if r:
            raise RuntimeError("solo_batch_reset -> %d" % r)

    _WHICH = {"enc": 1, "encoder": 1, "dec": 2, "decoder": 2, "both": 3, 1: 1, 2: 2, 3: 3}

    def _subset(self, streams):
        """streams= of encode / decode / recv_decode: a sequence or an int32 CUDA tensor of stream indices, strictly increasing ->
        (int32 tensor on the device, n).  Checked here (the library checks the device list once more and refuses
        a bad one with status -1, but by then the call is enqueued).  While the current stream is capturing a graph a CUDA tensor
        is taken as it is -- reading it would synchronise, and a replay brings other contents anyway: the device check is the check."""
        t = self.torch
        on_dev = getattr(streams, "is_cuda", False)
        if on_dev and (streams.dtype != t.int32 or len(streams.shape) != 1):     # (need not be contiguous: it is made so below)
            raise ValueError("streams: a sequence or a 1-D int32 CUDA tensor")
        if on_dev and t.cuda.is_initialized() and t.cuda.is_current_stream_capturing():
            if not streams.is_contiguous() or not 0 < streams.shape[0] <= self.n_streams:
                raise ValueError("streams: in a graph capture a contiguous int32 CUDA tensor of 1 .. %d indices" % self.n_streams)
            return streams, int(streams.shape[0])
        idx = _increasing("streams", streams, self.n_streams)
        if on_dev:
            return streams.contiguous(), len(idx)
        return t.tensor(idx, dtype=t.int32, device=self.device), len(idx)

    def _list_as_is(self, streams):
        """streams= of recv_report / export_streams / import_streams: a 1-D int32 CUDA tensor is taken as it is and checked on the
        device (a bad one is refused there), a sequence goes through _subset -> (int32 tensor on the device, n)"""
        if getattr(streams, "is_cuda", False):
            n, = _tensor("streams", streams, self.torch.int32, (None,))
            if not 0 < n <= self.n_streams:
                raise ValueError("streams: 1 .. %d indices" % self.n_streams)
            return streams, n
        return self._subset(streams)

    def _rows_of(self, streams):
        """streams= of a call -> (None, N) for every stream of the handle, else _subset(streams)"""
        return (None, self.n_streams) if streams is None else self._subset(streams)

    @staticmethod
    def _per_stream(v, n, name):
        if v is None or isinstance(v, (int, bool)) or (hasattr(v, "ndim") and v.ndim == 0):
            return [v] * n
        v = list(v.tolist() if hasattr(v, "tolist") else v)
        if len(v) != n:
            raise ValueError("%s: one value per listed stream (%d), got %d" % (name, n, len(v)))
        return v

    def _ctl_arrays(self, streams, rate, dtx, use_md_index, which):
        """the arguments of solo_batch_reset_streams / solo_batch_update_streams: (stream indices, which, encoder controls or None,
        decoder controls or None); None controls mean the handle's create-time control"""
        idx = _distinct("streams", streams, self.n_streams)
        n = len(idx)
        if which not in self._WHICH:
            raise ValueError("which must be 'enc', 'dec' or 'both'")
        w = self._WHICH[which]
        if which == "both":
            w = (1 if self._enc is not None else 0) | (2 if self._dec is not None else 0)
        if (w & 1 and self._enc is None) or (w & 2 and self._dec is None):
            raise ValueError("the handle has no %s" % ("encoder" if (w & 1 and self._enc is None) else "decoder"))
        rates, dtxs, mds = self._per_stream(rate, n, "rate"), self._per_stream(dtx, n, "dtx"), self._per_stream(use_md_index, n, "use_md_index")
        enc_arr = dec_arr = None
        if (rate is not None or dtx is not None) and not w & 1:
            raise ValueError("rate / dtx are encoder controls: the call does not reach an encoder")
        if w & 1 and (rate is not None or dtx is not None or use_md_index is not None):
            h = self._enc
            enc_arr = (USER_Ctrl_enc * n)()
            for i in range(n):
                r = h.targetRate_bps if rates[i] is None else int(rates[i])
                if h.samplerate == 32000 and (15600 if r <= 0 else r) - (800 if h.joint_enable and h.joint_mode == 1 else 1600) < 14000:
                    raise ValueError("the 32 kHz mode needs a rate that leaves SILK >= 14000 bps (stream %d: %d)" % (idx[i], r))
                enc_arr[i] = USER_Ctrl_enc(mode=h.mode, targetRate_bps=r, samplerate=h.samplerate,
                                           dtx_enable=h.dtx_enable if dtxs[i] is None else (1 if dtxs[i] else 0), framesize_ms=h.framesize_ms,
                                           joint_enable=h.joint_enable, joint_mode=h.joint_mode,
                                           useMDIndex=h.useMDIndex if mds[i] is None else int(mds[i]))
        if w & 2 and use_md_index is not None:
            h = self._dec
            dec_arr = (USER_Ctrl_dec * n)()
            for i in range(n):
                dec_arr[i] = USER_Ctrl_dec(packetLoss_perc=h.packetLoss_perc, samplerate=h.samplerate, framesize_ms=h.framesize_ms,
                                           joint_enable=h.joint_enable, joint_mode=h.joint_mode,
                                           useMDIndex=h.useMDIndex if mds[i] is None else int(mds[i]))
        return idx, w, enc_arr, dec_arr

    def reset_streams(self, streams, rate=None, dtx=None, use_md_index=None, which="both"):
        """Re-initialise the listed streams (solo_batch_reset_streams), each as a fresh encoder / decoder with its own control.  rate,
        dtx and use_md_index take a scalar or one value per listed stream; None means the handle's create-time value.  rate and dtx
        are encoder fields, use_md_index goes to both directions.  which: "enc" (1), "dec" (2) or "both" (3; on a handle of one
        direction: that direction).  Other streams are untouched; work enqueued on the current stream afterwards sees the new states."""
        idx, w, enc_arr, dec_arr = self._ctl_arrays(streams, rate, dtx, use_md_index, which)
        n = len(idx)
        r = self.lib.solo_batch_reset_streams(self.h, (C.c_int32 * n)(*idx), n, w, enc_arr, dec_arr, self._stream())
        if r:
            raise RuntimeError("solo_batch_reset_streams -> %d" % r)

    def update_streams(self, streams, rate=None, dtx=None, use_md_index=None, which="both"):
        """Change the control of the listed RUNNING streams (solo_batch_update_streams): the encoder's rate, DTX and useMDIndex, the
        decoder's useMDIndex; nothing else of their state, queue or play-out position changes.  Arguments as reset_streams (None: the
        handle's create-time value).  The new control applies from the next packet encoded / decoded on the current stream; packets
        of earlier calls keep the old one."""
        idx, w, enc_arr, dec_arr = self._ctl_arrays(streams, rate, dtx, use_md_index, which)
        n = len(idx)
        r = self.lib.solo_batch_update_streams(self.h, (C.c_int32 * n)(*idx), n, w, enc_arr, dec_arr, self._stream())
        if r:
            raise RuntimeError("solo_batch_update_streams -> %d" % r)

    RATES_COUNT = tuple(n for n, _ in solo_rate_apply_count_t._fields_)

    def update_rates(self, target, streams=None):
        """The rate of RUNNING streams from device memory (solo_batch_update_rates): target int32 [n] on the device, one value per stream
        (streams=None: n = N) or per listed stream (streams: a strictly increasing sequence or int32 CUDA tensor, as in encode()).  A
        value <= 0 keeps the stream as it is; a positive one is the `rate` of update_streams(), and nothing but the rate changes; on a
        32 kHz handle a value that leaves SILK below 14000 bps is refused for that stream alone.  This is what Rate.update() writes.
        -> count int32 [4] on the device, read with rates_count().  The new rate applies from the next packet encoded on the current
        stream; no synchronisation."""
        t = self.torch
        if self._enc is None:
            raise ValueError("the handle has no encoder")
        smap, n = self._rows_of(streams)
        _tensor("target", target, t.int32, (n,))
        count = t.zeros((4,), dtype=t.int32, device=target.device)
        r = self.lib.solo_batch_update_rates(self.h, _ptr(smap), n, target.data_ptr(), count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_batch_update_rates -> %d" % r)
        return count

    def rates_count(self, count):
        """the count tensor of update_rates() as a dict (synchronises): applied, kept, refused, listed; applied == -1: the stream list
        was refused on the device"""
        return _counts(solo_rate_apply_count_t, count)

    def encode(self, pcm, bits=None, nbytes=None, status=None, streams=None):
        """pcm: int16 CUDA tensor [N, P, 640] -> (bits uint8 [N,P,slot], nbytes int16 [N,P,2], status int32 [N]).
        streams: encode only these streams (solo_batch_encode_streams); every shape then has n = len(streams) rows in place of N,
        row i belonging to streams[i]; the other streams keep their state."""
        t = self.torch
        N, P, _ = _tensor("pcm", pcm, t.int16, (None, None, self.packet_samples))
        smap, n = self._rows_of(streams)
        if N != n or P < 1:
            raise ValueError("pcm: %d rows and at least one packet" % n)
        _tensor("bits", bits, t.uint8, (N, P, self.slot), optional=True)
        _tensor("nbytes", nbytes, t.int16, (N, P, 2), optional=True)
        _tensor("status", status, t.int32, (N,), optional=True)
        if bits is None:
            bits = t.zeros((N, P, self.slot), dtype=t.uint8, device=pcm.device)
        if nbytes is None:
            nbytes = t.zeros((N, P, 2), dtype=t.int16, device=pcm.device)
        if status is None:
            status = t.zeros((N,), dtype=t.int32, device=pcm.device)
        if smap is not None:
            r = self.lib.solo_batch_encode_streams(self.h, smap.data_ptr(), N, pcm.data_ptr(), P, bits.data_ptr(), nbytes.data_ptr(), status.data_ptr(),
                                                   self._stream())
            # (the handle's internal streams read the list: with asynchronous joins it must outlive the call, like its other inputs)
            self._enc_lists = (getattr(self, "_enc_lists", (None,))[-1], smap)
        else:
            r = self.lib.solo_batch_encode(self.h, pcm.data_ptr(), P, bits.data_ptr(), nbytes.data_ptr(), status.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_batch_encode%s -> %d" % ("_streams" if smap is not None else "", r))
        return bits, nbytes, status

    def set_timing(self, on=True):
        """Bracket every kernel launch with HIP events (benchmarks only)."""
        if self.lib.solo_batch_set_timing(self.h, 1 if on else 0):
            raise RuntimeError("solo_batch_set_timing failed")

    def last_kernel_ms(self):
        """{analysis, quantiser, coding, decode} durations (ms) of the most recent encode / decode call (synchronises)."""
        ms = (C.c_float * 4)()
        if self.lib.solo_batch_last_kernel_ms(self.h, ms):
            raise RuntimeError("solo_batch_last_kernel_ms failed")
        return dict(zip(("analysis", "quantiser", "coding", "decode"), [float(v) for v in ms]))

    def set_async_join(self, on):
        """encode() returns without joining its internal streams into the caller's stream (see solo_batch_set_async_join)"""
        if self.lib.solo_batch_set_async_join(self.h, 1 if on else 0):
            raise RuntimeError("solo_batch_set_async_join failed")

    def wait_encode(self, which=0):
        """make the current stream wait for an encode call: which = 0 the most recent one, 1 the one before"""
        if self.lib.solo_batch_wait_encode(self.h, self._stream(), int(which)):
            raise RuntimeError("solo_batch_wait_encode failed")

    def last_encode_chunks(self):
        """launches per encoder kernel of the most recent encode call (the call's packets are pipelined in chunks)"""
        return int(self.lib.solo_batch_last_encode_chunks(self.h))

    def decode(self, bits, nbytes, recv=None, pcm=None, status=None, streams=None):
        """bits uint8 [N,P,slot], nbytes int16 [N,P,2], recv uint8 [N,P] (bit0 MD1, bit1 MD2) -> pcm int16 [N,P,640] (1280 in the 32 kHz mode).
        streams: decode only these streams (solo_batch_decode_streams): n = len(streams) rows in place of N."""
        t = self.torch
        N, P, _ = _tensor("bits", bits, t.uint8, (None, None, self.slot))
        smap, n = self._rows_of(streams)
        if N != n or P < 1:
            raise ValueError("bits: %d rows and at least one packet" % n)
        _tensor("nbytes", nbytes, t.int16, (N, P, 2))
        _tensor("recv", recv, t.uint8, (N, P), optional=True)
        _tensor("pcm", pcm, t.int16, (N, P, self.packet_samples), optional=True)
        _tensor("status", status, t.int32, (N,), optional=True)
        if pcm is None:
            pcm = t.zeros((N, P, self.packet_samples), dtype=t.int16, device=bits.device)
        if status is None:
            status = t.zeros((N,), dtype=t.int32, device=bits.device)
        if smap is not None:
            r = self.lib.solo_batch_decode_streams(self.h, smap.data_ptr(), N, bits.data_ptr(), nbytes.data_ptr(), _ptr(recv), P, pcm.data_ptr(),
                                                   status.data_ptr(), self._stream())
        else:
            r = self.lib.solo_batch_decode(self.h, bits.data_ptr(), nbytes.data_ptr(), _ptr(recv), P, pcm.data_ptr(), status.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_batch_decode%s -> %d" % ("_streams" if smap is not None else "", r))
        return pcm, status

    def decode_split(self, desc_a, len_a, desc_b, len_b, pcm=None, status=None):
        """Receiver front end: the two descriptions of every packet in two arrival slots.  desc_a / desc_b uint8 [N,P,S],
        len_a / len_b int16 [N,P] (0 = nothing arrived) -> pcm int16 [N,P,640] (see solo_batch_decode_split)."""
        t = self.torch
        N, P, S = _tensor("desc_a", desc_a, t.uint8, (self.n_streams, None, None))
        if P < 1:
            raise ValueError("desc_a: at least one packet")
        _tensor("desc_b", desc_b, t.uint8, (N, P, S))
        _tensor("len_a", len_a, t.int16, (N, P))
        _tensor("len_b", len_b, t.int16, (N, P))
        _tensor("pcm", pcm, t.int16, (N, P, self.packet_samples), optional=True)
        _tensor("status", status, t.int32, (N,), optional=True)
        if pcm is None:
            pcm = t.zeros((N, P, self.packet_samples), dtype=t.int16, device=desc_a.device)
        if status is None:
            status = t.zeros((N,), dtype=t.int32, device=desc_a.device)
        r = self.lib.solo_batch_decode_split(self.h, desc_a.data_ptr(), len_a.data_ptr(), desc_b.data_ptr(), len_b.data_ptr(), S, P,
                                             pcm.data_ptr(), status.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_batch_decode_split -> %d" % r)
        return pcm, status

    # ---- receiver staging ring (solo_recv_*: the reference README's "cache queue", sequence-indexed) ----
    RECV_STATS = ("inserted", "late", "ahead", "duplicate", "bad")

    def recv_create(self, depth, slot_bytes=256, first_seq=0):
        r = self.lib.solo_recv_create(self.h, depth, slot_bytes, first_seq, self._stream())
        if r:
            raise RuntimeError("solo_recv_create -> %d" % r)

    def recv_insert(self, arrivals, payload):
        """arrivals: int32 [n,5] (stream, seq, desc, offset, len) on the device; payload: uint8 [bytes] on the device."""
        t = self.torch
        n, _ = _tensor("arrivals", arrivals, t.int32, (None, 5))
        nbytes, = _tensor("payload", payload, t.uint8, (None,))
        r = self.lib.solo_recv_insert(self.h, arrivals.data_ptr(), n, payload.data_ptr(), nbytes, self._stream())
        if r:
            raise RuntimeError("solo_recv_insert -> %d" % r)

    def recv_decode(self, n_packets=1, pcm=None, status=None, streams=None):
        """Decode the next n_packets sequence numbers of every stream from what has arrived -> pcm int16 [N,n_packets,samples].
        streams: play out only these streams (solo_recv_decode_streams): pcm [n,n_packets,samples], status [n]; the others keep
        their queue and play-out position."""
        t = self.torch
        try:
            n_packets = operator.index(n_packets)
        except TypeError:
            n_packets = 0
        if n_packets < 1:
            raise ValueError("n_packets: a positive int")
        smap, N = self._rows_of(streams)
        _tensor("pcm", pcm, t.int16, (N, n_packets, self.packet_samples), optional=True)
        _tensor("status", status, t.int32, (N,), optional=True)
        if pcm is None:
            pcm = t.zeros((N, n_packets, self.packet_samples), dtype=t.int16, device=self.device)
        if status is None:
            status = t.zeros((N,), dtype=t.int32, device=self.device)
        if smap is not None:
            r = self.lib.solo_recv_decode_streams(self.h, smap.data_ptr(), N, n_packets, pcm.data_ptr(), status.data_ptr(), self._stream())
        else:
            r = self.lib.solo_recv_decode(self.h, n_packets, pcm.data_ptr(), status.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_recv_decode%s -> %d" % ("_streams" if smap is not None else "", r))
        return pcm, status

    def recv_reset_streams(self, streams, first_seq):
        """Empty the staging queue of the listed streams and set their play-out positions (solo_recv_reset_streams); first_seq: a
        scalar or one sequence number (>= 0) per listed stream.  Statistics and the other streams are untouched."""
        idx = _distinct("streams", streams, self.n_streams)
        seqs = [int(v) for v in self._per_stream(first_seq, len(idx), "first_seq")]
        if any(v < 0 for v in seqs):
            raise ValueError("first_seq must be >= 0")
        n = len(idx)
        r = self.lib.solo_recv_reset_streams(self.h, (C.c_int32 * n)(*idx), n, (C.c_int32 * n)(*seqs), self._stream())
        if r:
            raise RuntimeError("solo_recv_reset_streams -> %d" % r)

    def recv_stats(self):
        out = (C.c_uint32 * 8)()
        r = self.lib.solo_recv_stats(self.h, out, self._stream())
        if r:
            raise RuntimeError("solo_recv_stats -> %d" % r)
        return dict(zip(self.RECV_STATS, list(out)[:5]))

    # ---- read side of the ring (solo_recv_track, solo_recv_report): per-stream queue report, counters, play-out list ----
    RECV_REPORT = tuple(f[0] for f in solo_recv_report_t._fields_)

    def recv_track(self, on=True):
        """Per-stream counting of arrivals and played packets (solo_recv_track): on zeroes the counters and starts, off stops and keeps
        the values.  Off by default; while off insert and play-out enqueue exactly what they always did."""
        r = self.lib.solo_recv_track(self.h, 1 if on else 0, self._stream())
        if r:
            raise RuntimeError("solo_recv_track -> %d" % r)

    def recv_report(self, streams=None, min_ready=0, max_span=0, clear_margin=False, reports=None, play_list=None, play_rows=None):
        """What is queued per stream, its counters, and the streams that are ready to play (solo_recv_report) -> (reports int32 [n,16] with
        the columns RECV_REPORT, play_list int32 [n], play_rows int32 [n], count int32 [2] on the device: read it with
        recv_report_count()).  streams: None = all, a strictly increasing sequence, or a 1-D int32 CUDA tensor (taken as it is and
        checked on the device: a bad one gives selected = -1).  Row i is selected when ready >= min_ready (an int, or an int32 CUDA
        tensor [n] with one threshold per row; <= 0 selects always) or when max_span > 0 and span >= max_span.  play_list[:selected] is
        what recv_decode(streams=...) takes.  clear_margin: margin_min of the listed streams starts afresh after this report.
        Enqueued on the current stream, no synchronisation."""
        t = self.torch
        smap, n = (None, self.n_streams) if streams is None else self._list_as_is(streams)
        mr_v, mr = None, 0
        if isinstance(min_ready, int) and not isinstance(min_ready, bool):
            mr = min_ready
        else:
            _tensor("min_ready (unless an int)", min_ready, t.int32, (n,))
            mr_v = min_ready
        max_span = int(max_span)
        if not (-2 ** 31 <= mr < 2 ** 31 and -2 ** 31 <= max_span < 2 ** 31):
            raise ValueError("min_ready / max_span must fit int32")
        _tensor("reports", reports, t.int32, (n, 16), optional=True)
        _tensor("play_list", play_list, t.int32, (n,), optional=True)
        _tensor("play_rows", play_rows, t.int32, (n,), optional=True)
        if reports is None:
            reports = t.zeros((n, 16), dtype=t.int32, device=self.device)
        if play_list is None:
            play_list = t.zeros((n,), dtype=t.int32, device=self.device)
        if play_rows is None:
            play_rows = t.zeros((n,), dtype=t.int32, device=self.device)
        count = t.zeros((2,), dtype=t.int32, device=self.device)
        r = self.lib.solo_recv_report(self.h, _ptr(smap), n, _ptr(mr_v), mr, max_span, RECV_REPORT_CLEAR_MARGIN if clear_margin else 0,
                                      reports.data_ptr(), play_list.data_ptr(), play_rows.data_ptr(), count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_recv_report -> %d" % r)
        return reports, play_list, play_rows, count

    def recv_report_count(self, count):
        """the count tensor of recv_report() as a dict (synchronises): selected rows, listed rows; selected == -1: the stream list was
        refused on the device"""
        return _counts(solo_recv_report_count_t, count)

    # ---- sender back end (solo_send_pack): slots + length records -> datagram records + a dense payload pool ----
    SEND_COUNT = tuple(n for n, _ in solo_send_count_t._fields_)

    def send_pack(self, bits, nbytes, send=None, first_seq=0, seq_base=None, records=None, payload=None, streams=None):
        """What encode() wrote -> the datagrams to send: bits uint8 [n,P,slot], nbytes int16 [n,P,2], send uint8 [n,P] (bit 0: MD1, bit 1:
        MD2 || HB; None = both), seq_base int32 [n] or None -> (records int32 [max,5] = (stream, seq, desc, offset, len) per datagram,
        payload uint8 [cap], count int32 [8] on the device: read it with send_count()).  Packet p of row i has the sequence number
        first_seq + seq_base[i] + p; the order is packet-major, then row, then description.  records / payload: the caller's buffers
        (their sizes are the caps; what does not fit is counted, not written); the defaults, 2*n*P records and n*P*slot bytes, never
        overflow.  streams: the rows are these streams (solo_send_pack_streams), as in encode().  The records and the pool are what
        recv_insert() of the receiving handle takes.  Enqueued on the current stream, no synchronisation; with asynchronous joins call
        wait_encode() first."""
        t = self.torch
        n, P, S = _tensor("bits", bits, t.uint8, (None, None, self.slot))
        _tensor("nbytes", nbytes, t.int16, (n, P, 2))
        smap, k = self._rows_of(streams)
        if n != k or P < 1:
            raise ValueError("bits: %d rows and at least one packet" % k)
        _tensor("send", send, t.uint8, (n, P), optional=True)
        _tensor("seq_base", seq_base, t.int32, (n,), optional=True)
        if 2 * n * P >= 2 ** 31:
            raise ValueError("n * P * 2 must stay below 2^31")
        records, payload, count, out = self._send_out(first_seq, records, payload, 2 * n * P, n * P * S, bits)
        tail = (bits.data_ptr(), nbytes.data_ptr(), _ptr(send), P, _ptr(seq_base)) + out + (self._stream(),)
        if smap is not None:
            r = self.lib.solo_send_pack_streams(self.h, smap.data_ptr(), n, *tail)
        else:
            r = self.lib.solo_send_pack(self.h, *tail)
        if r:
            raise RuntimeError("solo_send_pack%s -> %d" % ("_streams" if smap is not None else "", r))
        return records, payload, count

    def _send_out(self, first_seq, records, payload, max_records, capacity, bits):
        """what send_pack() and send_fanout() share: first_seq fits int32; records int32 [max, 5] and payload uint8 [cap] are the
        caller's or, by default, max_records and capacity large, on the device of bits -> (records, payload, count int32 [8], the
        arguments of the library from first_seq to d_count)"""
        t = self.torch
        first_seq = int(first_seq)
        if not -2 ** 31 <= first_seq < 2 ** 31:
            raise ValueError("first_seq must fit int32")
        _tensor("records", records, t.int32, (None, 5), optional=True)
        _tensor("payload", payload, t.uint8, (None,), optional=True)
        if records is None:
            records = t.zeros((max_records, 5), dtype=t.int32, device=bits.device)
        if payload is None:
            payload = t.zeros((capacity,), dtype=t.uint8, device=bits.device)
        count = t.zeros((8,), dtype=t.int32, device=bits.device)
        # (an empty tensor has no address: a cap of 0 only counts, the pointer is never used -- the library still wants one)
        return records, payload, count, (first_seq, records.data_ptr() or count.data_ptr(), records.shape[0],
                                         payload.data_ptr() or count.data_ptr(), payload.shape[0], count.data_ptr())

    def send_count(self, count):
        """the count tensor of send_pack() as a dict (synchronises): records / bytes written, records_needed / bytes_needed without the
        caps, empty (DTX) and refused packets; records == -1: the stream list was refused on the device"""
        return _counts(solo_send_count_t, count)

    # ---- mixing bridge (solo_mix): decoded rows -> what every participant of a room hears ----
    MIX_COUNT = tuple(n for n, _ in solo_mix_count_t._fields_)

    def mix(self, pcm, room, gain=None, max_speakers=0, out=None, energy=None, mixed=None):
        """Mix-minus on the device: pcm int16 [n,P,samples] (what decode() / recv_decode() wrote, compact rows included), room int32 [n]
        (the room of row i, -1 = in none), gain int16 [n] in Q12 or None (= 4096; negative = muted) -> (out int16 [n,P,samples] = what
        encode() takes, count int32 [4] on the device: read it with mix_count()).  Every member of a room hears the sum of the others;
        with 0 < max_speakers (<= 64) < the room only the max_speakers loudest rows of each packet are mixed (larger energy first,
        then smaller row index).  Rows in no room keep their `out` (zeros when `out` is allocated here).  energy int64 [n,P] /
        mixed uint8 [n,P]: optional outputs, the energy of every member's contribution and whether it was mixed.  Room ids run up to
        n - 1 (a row is in one room, so n rooms are enough); an id outside [-1, n) refuses the call on the device: rows == -1 in
        the count, nothing else written.  Without a selection (max_speakers <= 0) at most 8191 rows.  Enqueued on the current stream,
        no synchronisation."""
        t = self.torch
        n, P, L = _tensor("pcm", pcm, t.int16, (None, None, self.packet_samples))
        if n <= 0 or P <= 0:
            raise ValueError("pcm: at least one row and one packet")
        if n * P >= 2 ** 31:
            raise ValueError("n * P must stay below 2^31")
        _tensor("room", room, t.int32, (n,))
        _tensor("gain", gain, t.int16, (n,), optional=True)
        max_speakers = int(max_speakers)
        if max_speakers > 64:
            raise ValueError("max_speakers: at most 64")
        if max_speakers <= 0 and n > 8191:
            raise ValueError("more than 8191 rows need 0 < max_speakers <= 64")
        _tensor("out", out, t.int16, (n, P, L), optional=True)
        _tensor("energy", energy, t.int64, (n, P), optional=True)
        _tensor("mixed", mixed, t.uint8, (n, P), optional=True)
        if out is None:
            out = t.zeros((n, P, L), dtype=t.int16, device=pcm.device)
        count = t.zeros((4,), dtype=t.int32, device=pcm.device)
        r = self.lib.solo_mix(self.h, pcm.data_ptr(), n, P, room.data_ptr(), n, _ptr(gain), max_speakers, out.data_ptr(), _ptr(energy), _ptr(mixed),
                              count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_mix -> %d" % r)
        return out, count

    def mix_count(self, count):
        """the count tensor of mix() as a dict (synchronises): rows that got an output, rooms with a member, saturated output samples;
        rows == -1: a room id was refused on the device"""
        return _counts(solo_mix_count_t, count)

    # ---- play-out time scaling (solo_timescale): a decoded packets of a row -> b packets of audio ----
    TIMESCALE_COUNT = tuple(n for n, _ in solo_timescale_count_t._fields_)

    def timescale(self, pcm, out_packets, out=None, shift=None, cost=None):
        """Shorten or stretch play-out by whole packets on the device: pcm int16 [n,a,samples] (what recv_decode() wrote, compact rows
        included), a and out_packets = b in 1 .. 4 -> (out int16 [n,b,samples] = what mix() / encode() take, count int32 [4] on the device:
        read it with timescale_count()).  Waveform-similarity overlap-add in integer arithmetic, per row and stateless; the first 5 ms and
        the last sample of a row are the input's, a == b is the identity (include/solo_mi355x.h has the arithmetic).  shift / cost int32
        [n, M], M = b * samples / (samplerate / 200) blocks of 5 ms: optional outputs, the lag every block was cut at and what its splice
        cost (the sum of absolute differences) -- the caller's quality gate.  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        n, a, L = _tensor("pcm", pcm, t.int16, (None, None, self.packet_samples))
        if n <= 0:
            raise ValueError("pcm: at least one row")
        b = int(out_packets)
        if not (1 <= a <= 4 and 1 <= b <= 4):
            raise ValueError("between 1 and 4 packets in and out")
        if n * max(a, b) * L >= 2 ** 31:
            raise ValueError("n * max(a, b) * samples must stay below 2^31")
        M = b * L // (self.samplerate // 200)
        _tensor("out", out, t.int16, (n, b, L), optional=True)
        _tensor("shift", shift, t.int32, (n, M), optional=True)
        _tensor("cost", cost, t.int32, (n, M), optional=True)
        if out is None:
            out = t.empty((n, b, L), dtype=t.int16, device=pcm.device)
        count = t.zeros((4,), dtype=t.int32, device=pcm.device)
        r = self.lib.solo_timescale(self.h, pcm.data_ptr(), n, a, b, out.data_ptr(), _ptr(shift), _ptr(cost), count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_timescale -> %d" % r)
        return out, count

    def timescale_count(self, count):
        """the count tensor of timescale() as a dict (synchronises): rows written, blocks searched, the sum of all splice costs"""
        return _counts(solo_timescale_count_t, count)

    # ---- shared listener mixes (solo_mix_shared, solo_send_fanout): a personal mix per speaker, one mix per room for everybody else ----
    MIX_SHARED_COUNT = tuple(n for n, _ in solo_mix_shared_count_t._fields_)

    def _shared_mix_args(self, pcm, room, gain, keep, slots, n_rooms, energy, pcm_spk, pcm_room):
        """the checks of the arguments mix_shared() and mix_selected() both take -> (n, P, samples, n_rooms)"""
        t = self.torch
        n, P, L = _tensor("pcm", pcm, t.int16, (None, None, self.packet_samples))
        if n <= 0 or P <= 0:
            raise ValueError("pcm: at least one row and one packet")
        if n * P >= 2 ** 31:
            raise ValueError("n * P must stay below 2^31")
        n_rooms = n if n_rooms is None else int(n_rooms)
        if not 0 < n_rooms <= n:
            raise ValueError("n_rooms: between 1 and the number of rows")
        _tensor("room", room, t.int32, (n,))
        _tensor("gain", gain, t.int16, (n,), optional=True)
        _tensor("keep", keep, t.uint8, (n,), optional=True)
        _tensor("slots", slots, t.int32, (n,), optional=True)
        _tensor("energy", energy, t.int64, (n, P), optional=True)
        _tensor("pcm_spk", pcm_spk, t.int16, (n, P, L), optional=True)
        _tensor("pcm_room", pcm_room, t.int16, (n_rooms, P, L), optional=True)
        return n, P, L, n_rooms

    def _shared_mix_outputs(self, device, n, P, L, n_rooms, pcm_spk, pcm_room):
        """the outputs mix_shared() and mix_selected() both return, the two PCM tables being the caller's or zeros ->
        (pcm_spk, spk_list, spk_rows, pcm_room, room_list, source)"""
        t = self.torch
        z = lambda shape, dt: t.zeros(shape, dtype=dt, device=device)
        if pcm_spk is None:
            pcm_spk = z((n, P, L), t.int16)
        if pcm_room is None:
            pcm_room = z((n_rooms, P, L), t.int16)
        return pcm_spk, z((n,), t.int32), z((n,), t.int32), pcm_room, z((n_rooms,), t.int32), z((n,), t.int32)

    def mix_shared(self, pcm, room, gain=None, max_speakers=3, keep=None, slots=None, n_rooms=None, energy=None, mixed=None, pcm_spk=None,
                   pcm_room=None):
        """solo_mix_shared: pcm int16 [n,P,samples], room int32 [n], gain int16 [n] or None as for mix(); max_speakers in [1, 64];
        keep uint8 [n] or None (non-zero: the row stays a speaker of the call whether it is picked or not); slots int32 [n] or None (row ->
        transmit slot, strictly increasing; None = the row index); n_rooms: room ids run up to n_rooms - 1 (default n) ->
        (pcm_spk int16 [n,P,samples], spk_list int32 [n], spk_rows int32 [n], pcm_room int16 [n_rooms,P,samples], room_list int32 [n_rooms],
        source int32 [n], count int32 [6] on the device: read it with mix_shared_count()).  Only the first `speakers` rows of pcm_spk /
        spk_list / spk_rows and the first `shared` rows of pcm_room / room_list are written: pcm_spk[:speakers] is what encode(streams=
        spk_list[:speakers]) takes on the participants' handle, pcm_room[:shared] what encode(streams=room_list[:shared]) takes on a
        handle with one slot per room; with both results in one table (speakers in rows 0.., rooms in rows n..) `source` is the source
        of send_fanout().  A room id outside [-1, n_rooms) or slots that do not grow strictly from a non-negative start refuse the call
        on the device: rows == -1 in the count, nothing else written.  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        max_speakers = int(max_speakers)
        if not 1 <= max_speakers <= 64:
            raise ValueError("max_speakers: between 1 and 64")
        n, P, L, n_rooms = self._shared_mix_args(pcm, room, gain, keep, slots, n_rooms, energy, pcm_spk, pcm_room)
        _tensor("mixed", mixed, t.uint8, (n, P), optional=True)
        pcm_spk, spk_list, spk_rows, pcm_room, room_list, source = self._shared_mix_outputs(pcm.device, n, P, L, n_rooms, pcm_spk, pcm_room)
        count = t.zeros((6,), dtype=t.int32, device=pcm.device)
        r = self.lib.solo_mix_shared(self.h, pcm.data_ptr(), n, P, room.data_ptr(), n_rooms, _ptr(gain), max_speakers, _ptr(keep), _ptr(slots),
                                     pcm_spk.data_ptr(), spk_list.data_ptr(), spk_rows.data_ptr(), pcm_room.data_ptr(), room_list.data_ptr(),
                                     source.data_ptr(), _ptr(energy), _ptr(mixed), count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_mix_shared -> %d" % r)
        return pcm_spk, spk_list, spk_rows, pcm_room, room_list, source, count

    def mix_shared_count(self, count):
        """the count tensor of mix_shared() as a dict (synchronises): rows in a room, rooms with a member, speakers (rows of pcm_spk
        written), shared (rows of pcm_room written), saturated samples among them; rows == -1: the call was refused on the device"""
        return _counts(solo_mix_shared_count_t, count)

    # ---- shared listener mixes from a given selection (solo_mix_selected): the end of a tick that ran Vad.select ----
    MIX_SELECTED_COUNT = tuple(n for n, _ in solo_mix_selected_count_t._fields_)

    def mix_selected(self, pcm, room, sel, gain=None, keep=None, slots=None, n_rooms=None, energy=None, room_nsel=None, pcm_spk=None,
                     pcm_room=None):
        """solo_mix_selected: mix_shared() for a selection the caller brings.  pcm int16 [n,P,samples], room int32 [n], sel uint8 [n,P] (the
        tensor Vad.select returns: non-zero = row i speaks in packet p; a room may have no speaker, or only speakers; at most 64 per room
        and packet), gain int16 [n] or None (the callers' own gains), keep / slots / n_rooms as for mix_shared() ->
        (pcm_spk, spk_list, spk_rows, pcm_room, room_list, source, count int32 [8] on the device: read it with mix_selected_count(),
        room_nsel uint8 [n_rooms,P]).  The first seven are what mix_shared() returns, with its layouts; room_nsel[j, p] (first `shared`
        rows) is the number of speakers of the j-th shared room in packet p: 0 = that packet of pcm_room[j] is digital silence, which
        the caller may leave unsent (the send mask of send_fanout()).  energy int64 [n,P]: optional output, solo_mix's energies; without
        it the input is never read for them.  A room id outside [-1, n_rooms), slots that do not grow strictly from a non-negative start
        or more than 64 selected rows in a room and packet refuse the call on the device: rows == -1 in the count, nothing else written.
        Enqueued on the current stream, no synchronisation."""
        t = self.torch
        n, P, L, n_rooms = self._shared_mix_args(pcm, room, gain, keep, slots, n_rooms, energy, pcm_spk, pcm_room)
        _tensor("sel", sel, t.uint8, (n, P))
        _tensor("room_nsel", room_nsel, t.uint8, (n_rooms, P), optional=True)
        pcm_spk, spk_list, spk_rows, pcm_room, room_list, source = self._shared_mix_outputs(pcm.device, n, P, L, n_rooms, pcm_spk, pcm_room)
        if room_nsel is None:
            room_nsel = t.zeros((n_rooms, P), dtype=t.uint8, device=pcm.device)
        count = t.zeros((8,), dtype=t.int32, device=pcm.device)
        r = self.lib.solo_mix_selected(self.h, pcm.data_ptr(), n, P, room.data_ptr(), n_rooms, _ptr(gain), sel.data_ptr(), _ptr(keep), _ptr(slots),
                                       pcm_spk.data_ptr(), spk_list.data_ptr(), spk_rows.data_ptr(), pcm_room.data_ptr(), room_list.data_ptr(),
                                       source.data_ptr(), room_nsel.data_ptr(), _ptr(energy), count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_mix_selected -> %d" % r)
        return pcm_spk, spk_list, spk_rows, pcm_room, room_list, source, count, room_nsel

    def mix_selected_count(self, count):
        """the count tensor of mix_selected() as a dict (synchronises): the five counts of mix_shared_count(), selected ((row, packet) pairs
        selected among rows in a room) and silent ((shared room, packet) pairs nobody speaks in); rows == -1: refused on the device"""
        return _counts(solo_mix_selected_count_t, count)

    def send_fanout(self, bits, nbytes, source, dst_stream=None, send=None, first_seq=0, seq_base=None, records=None, payload=None):
        """solo_send_fanout: one table of encoded packets (bits uint8 [n_src,P,slot], nbytes int16 [n_src,P,2]), many destinations: source
        int32 [n_dst] (the table row destination i sends, -1 = nothing), dst_stream int32 [n_dst] or None (= i), send uint8 [n_dst,P] or
        None (= both descriptions), seq_base int32 [n_dst] or None -> (records int32 [max,5], payload uint8 [cap], count int32 [8] on the
        device: read it with send_count()).  Every source datagram is in the pool once; the records of destinations with one source carry
        the same offset, and recv_insert() of the receiving handle files them all.  Order: packet-major, then destination, then
        description.  records / payload: the caller's buffers (their sizes are the caps); the defaults, 2*n_dst*P records and
        n_src*P*slot bytes, never overflow.  A source outside [-1, n_src) refuses the call on the device: records == -1 in the count.
        Enqueued on the current stream, no synchronisation; with asynchronous joins call wait_encode() first."""
        t = self.torch
        n_src, P, S = _tensor("bits", bits, t.uint8, (None, None, self.slot))
        if P <= 0 or n_src <= 0:
            raise ValueError("bits: at least one row and one packet")
        _tensor("nbytes", nbytes, t.int16, (n_src, P, 2))
        n_dst, = _tensor("source", source, t.int32, (None,))
        if n_dst <= 0:
            raise ValueError("source: at least one destination")
        _tensor("dst_stream", dst_stream, t.int32, (n_dst,), optional=True)
        _tensor("send", send, t.uint8, (n_dst, P), optional=True)
        _tensor("seq_base", seq_base, t.int32, (n_dst,), optional=True)
        if 2 * n_dst * P >= 2 ** 31 or 2 * n_src * P >= 2 ** 31:
            raise ValueError("n_dst * P * 2 and n_src * P * 2 must stay below 2^31")
        records, payload, count, out = self._send_out(first_seq, records, payload, 2 * n_dst * P, n_src * P * S, bits)
        r = self.lib.solo_send_fanout(self.h, bits.data_ptr(), nbytes.data_ptr(), n_src, source.data_ptr(), _ptr(dst_stream), n_dst, _ptr(send), P,
                                      _ptr(seq_base), *out, self._stream())
        if r:
            raise RuntimeError("solo_send_fanout -> %d" % r)
        return records, payload, count

    # ---- stream migration (solo_batch_export_streams / solo_batch_import_streams): a running call moves between handles ----
    MIGRATE_COUNT = tuple(n for n, _ in solo_migrate_count_t._fields_)
    _MIGRATE = {"enc": 1, "encoder": 1, "dec": 2, "decoder": 2, "recv": 4, "ring": 4}

    def _migrate_which(self, which):
        """"enc", "dec", "both" (the directions the handle has), "recv", a combination ("dec+recv", ("enc", "recv")), or the bits 1 | 2 | 4"""
        if isinstance(which, int) and not isinstance(which, bool):
            w = which
        else:
            w = 0
            for name in (which.split("+") if isinstance(which, str) else which):
                name = name.strip()
                if name == "both":
                    w |= (1 if self._enc is not None else 0) | (2 if self._dec is not None else 0)
                elif name in self._MIGRATE:
                    w |= self._MIGRATE[name]
                else:
                    raise ValueError("which: 'enc', 'dec', 'both', 'recv' or a combination such as 'dec+recv'")
        if not 0 < w <= 7:
            raise ValueError("which names no section")
        return w

    def state_bytes(self, which="both"):
        """bytes of one exported record, header included (solo_batch_state_bytes): the smallest row stride of a blob"""
        r = int(self.lib.solo_batch_state_bytes(self.h, self._migrate_which(which)))
        if r < 0:
            raise ValueError("the handle lacks a direction or the receiver ring that `which` names")
        return r

    def export_streams(self, streams, which="both", blob=None):
        """The state of the listed streams as a device blob (solo_batch_export_streams) -> (blob uint8 [n, stride], count int32 [4] on the
        device: read it with migrate_count()).  which: "enc", "dec", "both", "recv" (the receive queue) or a combination ("dec+recv").
        Row i belongs to streams[i] (strictly increasing).  blob: the caller's buffer, contiguous, 16-byte aligned, stride >= state_bytes(which)
        and a multiple of 16.  The handle is only read.  The blob is valid for this library build only; sending it to another rank is a
        plain torch.distributed send of the tensor.  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        w = self._migrate_which(which)
        smap, n = self._list_as_is(streams)
        need = self.state_bytes(w)
        if blob is None:
            blob = t.zeros((n, need), dtype=t.uint8, device=self.device)
        else:
            _tensor("blob", blob, t.uint8, (n, None))
        count = t.zeros((4,), dtype=t.int32, device=self.device)
        r = self.lib.solo_batch_export_streams(self.h, smap.data_ptr(), n, w, blob.data_ptr(), blob.shape[1], count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_batch_export_streams -> %d" % r)
        return blob, count

    def import_streams(self, streams, blob, which="both"):
        """Row i of an exported blob becomes the state of streams[i] (solo_batch_import_streams) -> count int32 [4] on the device: read it with
        migrate_count().  Every record is checked on the device first (build, geometry, length, checksums); one bad record refuses the
        whole call -- streams == -1, refused = its index + 1 -- and the handle stays bit for bit as it was.  The imported streams keep
        their own rate, DTX and useMDIndex.  The blob may hold more sections than `which` takes."""
        t = self.torch
        w = self._migrate_which(which)
        smap, n = self._list_as_is(streams)
        _tensor("blob", blob, t.uint8, (n, None))
        count = t.zeros((4,), dtype=t.int32, device=self.device)
        r = self.lib.solo_batch_import_streams(self.h, smap.data_ptr(), n, w, blob.data_ptr(), blob.shape[1], count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_batch_import_streams -> %d" % r)
        return count

    def migrate_count(self, count):
        """the count tensor of export_streams() / import_streams() as a dict (synchronises): streams done, refused (import: index of the
        first bad record + 1), bytes written / taken; streams == -1: the call was refused on the device.  A refused EXPORT writes that word
        and nothing else: `refused` and `bytes` are then not defined by the library (0 here only because export_streams() hands it a
        zeroed count)"""
        return _counts(solo_migrate_count_t, count)

    def close(self):
        if getattr(self, "h", None):
            self.lib.solo_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _RowObject:
    """What Resampler, Vad, Playout, Agc and Rate share: a library object solo_<PREFIX>_* of n_rows state records on the current HIP device,
    carried from call to call, with its create / destroy / reset / reset_rows calls."""

    PREFIX = None

    def _create(self, *args):
        """the constructor's tail: solo_<PREFIX>_create(*args), after the subclass has checked them"""
        import torch
        self.h = None
        if not torch.cuda.is_available():
            raise RuntimeError("solo_amd needs a HIP device (MI355X); there is no CPU path")
        self.torch = torch
        self.lib = load_library()
        self.h = getattr(self.lib, "solo_%s_create" % self.PREFIX)(*args)
        if not self.h:
            raise RuntimeError("solo_%s_create failed (no GPU, or out of memory)" % self.PREFIX)
        self.device = torch.device("cuda", torch.cuda.current_device())

    def __del__(self):
        if getattr(self, "h", None):
            getattr(self.lib, "solo_%s_destroy" % self.PREFIX)(self.h)
            self.h = None

    def _stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def _call(self, name, *args, prefix=None):
        """solo_<PREFIX>_<name>(object, *args, stream); a refusal raises"""
        prefix = prefix or self.PREFIX
        r = getattr(self.lib, "solo_%s_%s" % (prefix, name))(self.h, *args, self._stream())
        if r:
            raise RuntimeError("solo_%s_%s -> %d" % (prefix, name, r))

    def _rows(self, rows, n=None):
        """None, or the list as a contiguous int32 CUDA tensor (a host sequence is checked here and copied)"""
        t = self.torch
        if rows is None:
            return None
        if not getattr(rows, "is_cuda", False):
            rows = t.tensor(_increasing("rows", rows, self.n_rows), dtype=t.int32, device=self.device)
        k, = _tensor("rows", rows, t.int32, (n,))
        if not 0 < k <= self.n_rows:
            raise ValueError("rows: 1 .. %d indices" % self.n_rows)
        return rows

    def _n(self, rows):
        return self.n_rows if rows is None else int(rows.shape[0])

    def reset(self, rows=None):
        """every row, or the listed rows (a host sequence: inside [0, n_rows), none twice), back to the initial state"""
        if rows is None:
            return self._call("reset")
        idx = _distinct("rows", rows, self.n_rows)
        self._call("reset_rows", (C.c_int32 * len(idx))(*idx), len(idx))


class _RowStateObject(_RowObject):
    """... whose records can be read and written (solo_<PREFIX>_get_state / _set_state): state_bytes a row"""

    state_bytes = None

    def get_state(self, rows=None):
        """the state of the listed rows (None: all rows) -> uint8 [n, state_bytes] on the device"""
        rows = self._rows(rows)
        n = self._n(rows)
        blob = self.torch.empty((n, self.state_bytes), dtype=self.torch.uint8, device=self.device)
        self._call("get_state", _ptr(rows), n, blob.data_ptr())
        return blob

    def set_state(self, blob, rows=None):
        """blob uint8 [n, state_bytes] on the device -> the state of the listed rows (None: rows 0 .. n-1)"""
        n, _ = _tensor("blob", blob, self.torch.uint8, (None, self.state_bytes))
        if not 0 < n <= self.n_rows:
            raise ValueError("blob: 1 .. %d records" % self.n_rows)
        self._call("set_state", _ptr(self._rows(rows, n)), n, blob.data_ptr())


RESAMPLE_PAIRS = ((48000, 16000), (48000, 32000), (32000, 16000), (16000, 8000), (16000, 32000), (8000, 16000), (16000, 48000), (32000, 48000))


class Resampler(_RowObject):
    """n_rows independent PCM rate converters on the current HIP device (solo_resample, include/solo_mi355x.h): the reference's
    fixed-point resampler bit for bit, its filter memory carried from call to call.  It sits between two handles of different rates,
    or between a handle and an 8 / 48 kHz endpoint; the pairs are RESAMPLE_PAIRS."""

    COUNT = ("rows", "listed")
    PREFIX = "resample"

    def __init__(self, n_rows, fs_in, fs_out):
        self.n_rows, self.fs_in, self.fs_out = int(n_rows), int(fs_in), int(fs_out)
        if self.n_rows <= 0:
            raise ValueError("n_rows must be positive")
        if (self.fs_in, self.fs_out) not in RESAMPLE_PAIRS:
            raise ValueError("fs_in -> fs_out must be one of %s" % ", ".join("%d->%d" % p for p in RESAMPLE_PAIRS))
        self._create(self.n_rows, self.fs_in, self.fs_out)

    def out_samples(self, in_samples):
        """samples per output packet of in_samples per input packet: in_samples * fs_out / fs_in; in_samples must be a positive multiple
        of 10 ms (fs_in / 100 samples)"""
        in_samples = int(in_samples)
        if in_samples <= 0 or in_samples % (self.fs_in // 100):
            raise ValueError("in_samples: a positive multiple of %d (10 ms at %d Hz)" % (self.fs_in // 100, self.fs_in))
        return in_samples // (self.fs_in // 100) * (self.fs_out // 100)

    def check(self, pcm, rows=None, out=None):
        """the argument checks of run() -> (n, P, in_samples, out_samples); rows: None or an int32 CUDA tensor"""
        t = self.torch
        n, P, L = _tensor("pcm", pcm, t.int16, (None, None, None))
        if n <= 0 or P <= 0:
            raise ValueError("pcm: at least one row and one packet")
        outs = self.out_samples(L)
        _tensor("rows", rows, t.int32, (n,), optional=True)
        if n > self.n_rows or (rows is None and n != self.n_rows):
            raise ValueError("pcm: %d rows, or at most as many with rows=" % self.n_rows)
        if n * P * max(L, outs) >= 2 ** 31:
            raise ValueError("n * P * samples must stay below 2^31")
        _tensor("out", out, t.int16, (n, P, outs), optional=True)
        return n, P, L, outs

    def run(self, pcm, rows=None, out=None):
        """pcm int16 [n,P,in_samples] at fs_in (what decode() / mix() wrote, compact rows included) -> out int16 [n,P,out_samples] at fs_out
        (what mix() / encode() take).  rows=None: n == n_rows, row i of the object converts row i.  rows = a sequence or an int32 CUDA tensor,
        strictly increasing: only those rows are converted, row i of pcm / out belongs to rows[i], the others keep their state; returns
        (out, count) with count int32 [2] on the device, read with count().  A bad list is refused on the device: rows == -1 in the
        count, nothing else written.  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        if rows is not None and not getattr(rows, "is_cuda", False):
            rows = t.tensor(_increasing("rows", rows, self.n_rows), dtype=t.int32, device=self.device)
        n, P, L, outs = self.check(pcm, rows, out)
        if out is None:
            out = t.empty((n, P, outs), dtype=t.int16, device=pcm.device)
        if rows is None:
            r = self.lib.solo_resample(self.h, pcm.data_ptr(), P, L, out.data_ptr(), self._stream())
            if r:
                raise RuntimeError("solo_resample -> %d" % r)
            return out
        count = t.zeros((2,), dtype=t.int32, device=pcm.device)
        r = self.lib.solo_resample_rows(self.h, rows.data_ptr(), n, pcm.data_ptr(), P, L, out.data_ptr(), count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_resample_rows -> %d" % r)
        return out, count

    def count(self, count):
        """the count tensor of run(rows=) as a dict (synchronises): rows converted, rows listed; rows == -1: the list was refused"""
        return _counts(solo_resample_count_t, count)


VAD_STATE_BYTES = 128


class Vad(_RowStateObject):
    """n_rows independent voice activity detectors on the current HIP device (solo_vad, include/solo_mi355x.h): the reference's
    fixed-point VAD bit for bit on frames of 160 or 320 samples, the RFC 6464 audio level of every packet, and a stateful speaker
    selection per room (solo_vad_select).  State carries from call to call."""

    COUNT = ("rows", "rooms", "selected", "changes")
    PREFIX, state_bytes = "vad", VAD_STATE_BYTES

    def __init__(self, n_rows, frame_samples):
        self.n_rows, self.frame = int(n_rows), int(frame_samples)
        if self.n_rows <= 0:
            raise ValueError("n_rows must be positive")
        if self.frame not in (160, 320):
            raise ValueError("frame_samples must be 160 or 320")
        self._create(self.n_rows, self.frame)

    def run(self, pcm, rows=None, detail=False, level=True):
        """pcm int16 [n,P,samples] (what decode() / mix() wrote; samples a multiple of frame_samples, at most 1920) -> dict(sa uint8 [n,P,F],
        detail int32 [n,P,F,6] = {SNR_dB_Q7, Tilt_Q15, Quality_Q15[4]} with detail=True, level uint8 [n,P] in -dBov with level=True, count
        int32 [4] on the device with rows=, read with count()).  rows=None: rows 0 .. n-1 of the object.  rows = a strictly increasing
        sequence or int32 CUDA tensor: row i of pcm belongs to rows[i], the others keep their state; a bad list is refused on the device:
        rows == -1 in the count, nothing else written.  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        n, P, L = _tensor("pcm", pcm, t.int16, (None, None, None))
        if not (0 < n <= self.n_rows and P > 0):
            raise ValueError("pcm: 1 .. %d rows and at least one packet" % self.n_rows)
        if L <= 0 or L % self.frame or L > 1920:
            raise ValueError("samples: a positive multiple of %d, at most 1920" % self.frame)
        rows = self._rows(rows, n)
        F = L // self.frame
        out = {"sa": t.empty((n, P, F), dtype=t.uint8, device=pcm.device)}
        if detail:
            out["detail"] = t.empty((n, P, F, 6), dtype=t.int32, device=pcm.device)
        if level:
            out["level"] = t.empty((n, P), dtype=t.uint8, device=pcm.device)
        if rows is not None:
            out["count"] = t.zeros((4,), dtype=t.int32, device=pcm.device)
        r = self.lib.solo_vad(self.h, _ptr(rows), n, pcm.data_ptr(), P, L, out["sa"].data_ptr(), _ptr(out.get("detail")), _ptr(out.get("level")),
                              _ptr(out.get("count")), self._stream())
        if r:
            raise RuntimeError("solo_vad -> %d" % r)
        return out

    def select(self, sa, level, room, n_rooms=None, max_speakers=3, on=128, off=64, hang=5, stick=6, gain=None, rows=None):
        """sa uint8 [n,P,F] and level uint8 [n,P] as run() wrote them, room int32 [n] (-1 = in no room; n_rooms=None: the largest id + 1,
        which synchronises) -> dict(sel uint8 [n,P], gain_out int16 [n] (what mix(gain=) takes: the row's gain if it is selected after the
        last packet, else 0), keep uint8 [n] (candidates: what mix_shared(keep=) takes), dominant int32 [n_rooms,P], count int32 [4],
        read with count()).  Entries of rows in no room are not written (they are zero here).  on / off: the thresholds on the largest SA_Q8
        of a packet for a silent / a talking row, hang: packets a row stays a candidate after it fell silent, stick: what an incumbent's
        key is raised by.  A room id outside [-1, n_rooms) or a bad list is refused on the device: rows == -1 in the count."""
        t = self.torch
        n, P, F = _tensor("sa", sa, t.uint8, (None, None, None))
        if not (0 < n <= self.n_rows and P > 0 and F > 0):
            raise ValueError("sa: 1 .. %d rows, at least one packet and one frame" % self.n_rows)
        _tensor("level", level, t.uint8, (n, P))
        _tensor("room", room, t.int32, (n,))
        _tensor("gain", gain, t.int16, (n,), optional=True)
        rows = self._rows(rows, n)
        if n_rooms is None:
            n_rooms = max(int(room.max()) + 1, 1)
        n_rooms = int(n_rooms)
        if not 0 < n_rooms <= self.n_rows:
            raise ValueError("n_rooms: 1 .. %d" % self.n_rows)
        prm = solo_vad_select_params_t(int(max_speakers), int(on), int(off), int(hang), int(stick))
        if not (1 <= prm.max_speakers <= 64 and 0 <= prm.off_q8 <= prm.on_q8 <= 255 and 0 <= prm.hang_packets <= 1000 and 0 <= prm.stick <= 127):
            raise ValueError("max_speakers 1 .. 64, 0 <= off <= on <= 255, hang 0 .. 1000, stick 0 .. 127")
        out = {"sel": t.zeros((n, P), dtype=t.uint8, device=sa.device), "gain_out": t.zeros((n,), dtype=t.int16, device=sa.device),
               "keep": t.zeros((n,), dtype=t.uint8, device=sa.device), "dominant": t.full((n_rooms, P), -1, dtype=t.int32, device=sa.device),
               "count": t.zeros((4,), dtype=t.int32, device=sa.device)}
        r = self.lib.solo_vad_select(self.h, _ptr(rows), n, sa.data_ptr(), level.data_ptr(), P, F, room.data_ptr(), n_rooms,
                                     C.byref(prm), _ptr(gain), out["sel"].data_ptr(), out["gain_out"].data_ptr(),
                                     out["keep"].data_ptr(), out["dominant"].data_ptr(), out["count"].data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_vad_select -> %d" % r)
        return out

    def count(self, count):
        """a count tensor of run(rows=) / select() as a dict (synchronises); rows == -1: the call was refused on the device"""
        return _counts(solo_vad_count_t, count)


PLAYOUT_STATE_BYTES = 128


class Playout(_RowStateObject):
    """Adaptive play-out delay control for n_rows streams on the current HIP device (solo_playout_*, include/solo_mi355x.h has the rule): per
    stream a 128-byte state record and one held packet; row s belongs to stream s of the SoloBatch it is ticked with.  tick() is the receive
    side of a bridge tick in one call; plan() and render() are its two stages alone."""

    ACTIONS = ("IDLE", "NORMAL", "HELD", "STRETCH", "ACCEL", "ACCEL_FORCED")
    OUTCOMES = tuple(f[0].upper() for f in solo_playout_render_count_t._fields_)
    PARAMS = dict(start_ready=2, max_span=0, window=16, tolerate=1, lo=1, hi=3, cooldown=8, cost_gate=0)
    PREFIX = "playout"

    def __init__(self, n_rows, packet_samples=PACKET_SAMPLES):
        self.n_rows, self.packet_samples = int(n_rows), int(packet_samples)
        if self.n_rows <= 0:
            raise ValueError("n_rows must be positive")
        if not 0 < self.packet_samples <= 1920 or self.packet_samples % 8:
            raise ValueError("packet_samples: a positive multiple of 8, at most 1920")
        self._create(self.n_rows, self.packet_samples)

    @property
    def state_bytes(self):
        """bytes per row of a get_state() / set_state() blob: the record, then the held packet"""
        return PLAYOUT_STATE_BYTES + 2 * self.packet_samples

    @classmethod
    def params(cls, **kw):
        """the policy as a solo_playout_params_t: PARAMS overridden by kw, range-checked as the library does"""
        unknown = set(kw) - set(cls.PARAMS)
        if unknown:
            raise ValueError("unknown play-out parameter(s): %s" % ", ".join(sorted(unknown)))
        v = dict(cls.PARAMS)
        for k, x in kw.items():
            try:
                v[k] = operator.index(x)
            except TypeError:
                raise ValueError("%s: an int" % k)
        if any(not -2 ** 31 <= x < 2 ** 31 for x in v.values()):
            raise ValueError("play-out parameters must fit int32")
        if not (v["start_ready"] >= 1 and v["max_span"] >= 0 and 1 <= v["window"] <= 32 and 0 <= v["tolerate"] <= 3 and 0 <= v["lo"] <= v["hi"] <= 64 and
                0 <= v["cooldown"] <= 1000):
            raise ValueError("start_ready >= 1, max_span >= 0, window 1 .. 32, tolerate 0 .. 3, 0 <= lo <= hi <= 64, cooldown 0 .. 1000")
        return solo_playout_params_t(*[v[k] for k, _ in solo_playout_params_t._fields_])

    def tick(self, batch, streams=None, **params):
        """The receive side of a tick (solo_playout_tick): report, plan, the two decodes, time scaling, render -> (heard int16 [n,samples],
        outcome int32 [n], status int32 [n], count int32 [12] on the device: read it with count()).  batch: the SoloBatch whose ring is
        played, with recv_track() on and as many streams as this object has rows.  streams: None = all, a strictly increasing sequence, or
        an int32 CUDA tensor (checked on the device: a bad one gives plan n_one = -1 and nothing else).  params: PARAMS overridden.
        Synchronises once (the 16-byte plan count)."""
        t = self.torch
        if not isinstance(batch, SoloBatch) or batch.n_streams != self.n_rows or batch.packet_samples != self.packet_samples:
            raise ValueError("batch: a SoloBatch of %d streams and %d samples a packet" % (self.n_rows, self.packet_samples))
        prm = self.params(**params)
        rows = self._rows(streams)
        n = self._n(rows)
        heard = t.zeros((n, self.packet_samples), dtype=t.int16, device=self.device)
        outcome = t.zeros((n,), dtype=t.int32, device=self.device)
        status = t.zeros((n,), dtype=t.int32, device=self.device)
        count = t.zeros((12,), dtype=t.int32, device=self.device)
        r = self.lib.solo_playout_tick(self.h, batch.h, _ptr(rows), n, C.byref(prm), heard.data_ptr(), outcome.data_ptr(), status.data_ptr(),
                                       count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_playout_tick -> %d" % r)
        return heard, outcome, status, count

    def plan(self, reports, depth, rows=None, **params):
        """reports int32 [n,16] as SoloBatch.recv_report() wrote them (tracking on, clear_margin=True), depth: the ring depth -> dict(action
        int32 [n], one / two / stretch_pos int32 [n] (compacted; the counts say how many entries count), count int32 [4], read with
        count()).  The first half of the state update; render() with the same rows must follow.  No synchronisation."""
        t = self.torch
        prm = self.params(**params)
        rows = self._rows(rows)
        n = self._n(rows)
        _tensor("reports", reports, t.int32, (n, 16))
        depth = int(depth)
        if not 0 < depth <= 4096:
            raise ValueError("depth: 1 .. 4096")
        out = {k: t.zeros((n,), dtype=t.int32, device=self.device) for k in ("action", "one", "two", "stretch_pos")}
        out["count"] = t.zeros((4,), dtype=t.int32, device=self.device)
        r = self.lib.solo_playout_plan(self.h, reports.data_ptr(), _ptr(rows), n, depth, C.byref(prm), out["action"].data_ptr(), out["one"].data_ptr(),
                                       out["two"].data_ptr(), out["stretch_pos"].data_ptr(), out["count"].data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_playout_plan -> %d" % r)
        return out

    def gather(self, pcm_one, stretch_pos, n_stretch):
        """rows stretch_pos[:n_stretch] of pcm_one int16 [n_one,samples] -> int16 [n_stretch,1,samples], what SoloBatch.timescale(., 2) takes"""
        t = self.torch
        n_one, _ = _tensor("pcm_one", pcm_one, t.int16, (None, self.packet_samples))
        k, = _tensor("stretch_pos", stretch_pos, t.int32, (None,))
        n_stretch = int(n_stretch)
        if not 0 < n_stretch <= min(k, n_one) or n_one > self.n_rows:
            raise ValueError("n_stretch: 1 .. min(len(stretch_pos), n_one), n_one at most %d" % self.n_rows)
        out = t.zeros((n_stretch, 1, self.packet_samples), dtype=t.int16, device=self.device)
        r = self.lib.solo_playout_gather(self.h, pcm_one.data_ptr(), n_one, stretch_pos.data_ptr(), n_stretch, out.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_playout_gather -> %d" % r)
        return out

    def render(self, action, block_samples, pcm_one=None, status_one=None, pcm_two=None, status_two=None, ts_stretch=None, cost_stretch=None,
               ts_accel=None, cost_accel=None, rows=None, **params):
        """The second stage (solo_playout_render): action int32 [n] of the plan() before, the decode outputs of its `one` list (pcm_one int16
        [n_one,samples], status_one int32 [n_one]) and `two` list (pcm_two [n_two,2,samples], status_two), the time scaler's outputs for
        the STRETCH rows (ts_stretch [n_stretch,2,samples], cost_stretch int32 [n_stretch,2M]) and the ACCEL rows (ts_accel
        [n_two,1,samples], cost_accel [n_two,M]), M = samples / block_samples; absent = an empty list -> (heard int16 [n,samples], outcome
        int32 [n], status int32 [n], count int32 [8], read with count()).  No synchronisation."""
        t = self.torch
        prm = self.params(**params)
        rows = self._rows(rows)
        n, L = self._n(rows), self.packet_samples
        _tensor("action", action, t.int32, (n,))
        block_samples = int(block_samples)
        if block_samples <= 0 or L % block_samples or L // block_samples > 16:
            raise ValueError("block_samples: a divisor of %d, at most 16 blocks a packet" % L)
        M = L // block_samples
        n_one = n_two = n_stretch = 0
        if pcm_one is not None or status_one is not None:
            n_one, _ = _tensor("pcm_one", pcm_one, t.int16, (None, L))
            _tensor("status_one", status_one, t.int32, (n_one,))
        if pcm_two is not None or status_two is not None or ts_accel is not None or cost_accel is not None:
            n_two, _, _ = _tensor("pcm_two", pcm_two, t.int16, (None, 2, L))
            _tensor("status_two", status_two, t.int32, (n_two,))
            _tensor("ts_accel", ts_accel, t.int16, (n_two, 1, L))
            _tensor("cost_accel", cost_accel, t.int32, (n_two, M))
        if ts_stretch is not None or cost_stretch is not None:
            n_stretch, _, _ = _tensor("ts_stretch", ts_stretch, t.int16, (None, 2, L))
            _tensor("cost_stretch", cost_stretch, t.int32, (n_stretch, 2 * M))
        if n_stretch > n_one or n_one + n_two > n:
            raise ValueError("n_stretch <= n_one and n_one + n_two <= n")
        heard = t.zeros((n, L), dtype=t.int16, device=self.device)
        outcome = t.zeros((n,), dtype=t.int32, device=self.device)
        status = t.zeros((n,), dtype=t.int32, device=self.device)
        count = t.zeros((8,), dtype=t.int32, device=self.device)

        def p(x, k):
            return _ptr(x) if k else None
        r = self.lib.solo_playout_render(self.h, _ptr(rows), n, C.byref(prm), block_samples, action.data_ptr(), n_one, n_two, n_stretch, p(pcm_one, n_one),
                                         p(status_one, n_one), p(pcm_two, n_two), p(status_two, n_two), p(ts_stretch, n_stretch), p(cost_stretch, n_stretch),
                                         p(ts_accel, n_two), p(cost_accel, n_two), heard.data_ptr(), outcome.data_ptr(), status.data_ptr(),
                                         count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_playout_render -> %d" % r)
        return heard, outcome, status, count

    def count(self, count):
        """a count tensor of plan() (4 words), render() (8) or tick() (12: dict(plan=..., render=...)) as a dict (synchronises)"""
        k, = _tensor("count", count, self.torch.int32, (None,))
        if k == 4:
            return _counts(solo_playout_plan_count_t, count)
        if k == 8:
            return _counts(solo_playout_render_count_t, count)
        if k != 12:
            raise ValueError("count: 4, 8 or 12 int32")
        return {"plan": _counts(solo_playout_plan_count_t, count[:4]), "render": _counts(solo_playout_render_count_t, count[4:])}

    def reset_rows(self, rows):
        """reset(rows): the listed rows (a host sequence: inside [0, n_rows), none twice) back to the initial state"""
        self.reset(rows)


AGC_STATE_BYTES = 64


class Agc(_RowStateObject):
    """n_rows independent level controls with a peak limiter on the current HIP device (solo_agc, include/solo_mi355x.h): every row's
    speech is brought to `target` -dBov with a slewed gain, and no output sample exceeds `ceiling`.  State carries from call to call."""

    COUNT = ("rows", "speech", "limited", "zero")
    PREFIX, state_bytes = "agc", AGC_STATE_BYTES

    def __init__(self, n_rows):
        self.n_rows = int(n_rows)
        if self.n_rows <= 0:
            raise ValueError("n_rows must be positive")
        self._create(self.n_rows)

    def run(self, pcm, level=None, sa=None, rows=None, out=None, target=23, boost=24, cut=12, sa_on=128, gate=50, alpha=32, up=128, down=256,
            ceiling=29204, release=256):
        """pcm int16 [n,P,samples] (samples a multiple of 32, 256 .. 1920), level uint8 [n,P] and sa uint8 [n,P,F] as Vad.run() wrote them
        (level=None: the level of the input samples, sa=None: activity 255) -> (pcm_out int16 [n,P,samples], level_out uint8 [n,P] in
        -dBov, gain_q8 int16 [n,P] in dB Q8, count int32 [4] on the device, read with count()).  out=: where pcm_out goes; out=pcm works in
        place.  target / gate: levels in -dBov; boost / cut: the gain's range in dB; sa_on: the activity a speech packet needs; alpha: the
        level's smoothing, Q8; up / down: the gain's slew per speech packet in dB Q8; ceiling: the largest output magnitude; release: what
        the limiter's envelope recovers per 32 samples, Q15.  rows as in Vad.run(): a bad list is refused on the device, rows == -1 in the
        count, nothing else written.  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        n, P, L = _tensor("pcm", pcm, t.int16, (None, None, None))
        if not (0 < n <= self.n_rows and P > 0):
            raise ValueError("pcm: 1 .. %d rows and at least one packet" % self.n_rows)
        if L % 32 or not 256 <= L <= 1920:
            raise ValueError("samples: a multiple of 32 inside 256 .. 1920")
        _tensor("level", level, t.uint8, (n, P), optional=True)
        F = _tensor("sa", sa, t.uint8, (n, P, None), optional=True)
        F = 0 if F is None else F[2]
        if sa is not None and F <= 0:
            raise ValueError("sa: at least one frame")
        _tensor("out", out, t.int16, (n, P, L), optional=True)
        rows = self._rows(rows, n)
        prm = solo_agc_params_t(int(target), int(boost), int(cut), int(sa_on), int(gate), int(alpha), int(up), int(down), int(ceiling), int(release))
        if not (0 <= prm.target_level <= 127 and 0 <= prm.max_boost_db <= 30 and 0 <= prm.max_cut_db <= 30 and 0 <= prm.sa_on_q8 <= 255 and
                0 <= prm.gate_level <= 127 and 1 <= prm.alpha_q8 <= 256 and 0 <= prm.slew_up_q8 <= 7680 and 0 <= prm.slew_down_q8 <= 7680 and
                1 <= prm.ceiling <= 32767 and 0 <= prm.release_q15 <= 32768):
            raise ValueError("target, gate 0 .. 127, boost, cut 0 .. 30, sa_on 0 .. 255, alpha 1 .. 256, up, down 0 .. 7680, ceiling 1 .. 32767, release 0 .. 32768")
        if out is None:
            out = t.empty_like(pcm)
        level_out = t.empty((n, P), dtype=t.uint8, device=pcm.device)
        gain = t.empty((n, P), dtype=t.int16, device=pcm.device)
        count = (t.empty if rows is None else t.zeros)((4,), dtype=t.int32, device=pcm.device)
        r = self.lib.solo_agc(self.h, _ptr(rows), n, pcm.data_ptr(), P, L, _ptr(level), _ptr(sa), F, C.byref(prm), out.data_ptr(), level_out.data_ptr(),
                              gain.data_ptr(), count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_agc -> %d" % r)
        return out, level_out, gain, count

    def count(self, count):
        """a count tensor of run() as a dict (synchronises); rows == -1: the list was refused on the device"""
        return _counts(solo_agc_count_t, count)


RATE_STATE_BYTES = 64


class Rate(_RowStateObject):
    """n_rows loss-based rate controllers on the current HIP device (solo_rate_*, include/solo_mi355x.h): update() turns the feedback rows
    of Rtcp.parse() into a target per stream for SoloBatch.update_rates() and a mode per stream, send_mask() turns the mode into the
    send= mask of SoloBatch.send_pack().  State carries from call to call."""

    COUNT = tuple(n for n, _ in solo_rate_count_t._fields_ if not n.startswith("reserved"))
    PREFIX, state_bytes = "rate", RATE_STATE_BYTES

    def __init__(self, n_rows):
        self.n_rows = int(n_rows)
        if self.n_rows <= 0:
            raise ValueError("n_rows must be positive")
        self._create(self.n_rows)

    def update(self, feedback, min_bps, max_bps, start_bps, quantum_bps=200, lo_q8=5, hi_q8=26, inc_q8=13, rtt_guard=0, stale_calls=250, thin_after=0,
               thin_release=3, target=None, mode=None):
        """feedback int32 [n_rows, 8] as Rtcp.parse() wrote it -> (target int32 [n_rows]: a row's new target in bps where it changed in
        this call, else 0; mode uint8 [n_rows]: 1 = one description per packet; count int32 [16] on the device, read with count()).
        The rates stay inside [min_bps, max_bps], multiples of quantum_bps, and begin at start_bps.  The other defaults are policy, not
        measurements: lo_q8 / hi_q8 / inc_q8 are the 2 % and 10 % loss thresholds and the 5 % step of the loss-based controller of the
        RMCAT "Google Congestion Control" draft; rtt_guard (1 / 65536 s above the smallest round trip seen; 0: off) holds increases;
        stale_calls without a report take the rate back to start_bps; thin_after (0: off) reports of loss at min_bps switch a row to one
        description per packet, thin_release clean ones switch it back.  target= / mode=: the caller's buffers (a captured call).
        Enqueued on the current stream, no synchronisation."""
        t = self.torch
        _tensor("feedback", feedback, t.int32, (self.n_rows, 8))
        _tensor("target", target, t.int32, (self.n_rows,), optional=True)
        _tensor("mode", mode, t.uint8, (self.n_rows,), optional=True)
        prm = solo_rate_params_t(int(min_bps), int(max_bps), int(start_bps), int(quantum_bps), int(lo_q8), int(hi_q8), int(inc_q8), int(rtt_guard),
                                 int(stale_calls), int(thin_after), int(thin_release), 0)
        q = prm.quantum_bps
        if not (q >= 1 and 1 <= prm.min_bps <= prm.start_bps <= prm.max_bps <= 1000000 and not (prm.min_bps % q or prm.max_bps % q or prm.start_bps % q) and
                0 <= prm.lo_q8 <= prm.hi_q8 <= 255 and 0 <= prm.inc_q8 <= 256 and min(prm.rtt_guard, prm.stale_calls, prm.thin_after, prm.thin_release) >= 0):
            raise ValueError("1 <= min_bps <= start_bps <= max_bps <= 1000000, all multiples of quantum_bps >= 1; 0 <= lo_q8 <= hi_q8 <= 255; inc_q8 0 .. 256; "
                             "rtt_guard, stale_calls, thin_after, thin_release >= 0")
        if feedback.data_ptr() & 15:
            raise ValueError("feedback: 16-byte aligned")
        if target is None:
            target = t.empty((self.n_rows,), dtype=t.int32, device=feedback.device)
        if mode is None:
            mode = t.empty((self.n_rows,), dtype=t.uint8, device=feedback.device)
        count = t.empty((16,), dtype=t.int32, device=feedback.device)
        self._call("update", feedback.data_ptr(), C.byref(prm), target.data_ptr(), mode.data_ptr(), count.data_ptr())
        return target, mode, count

    def send_mask(self, mode, n_packets, streams=None, seq_base=None, first_seq=0, send=None, out=None):
        """mode uint8 [n_rows] as update() wrote it -> the send= mask of SoloBatch.send_pack(), uint8 [n, n_packets]: 3 for a row in mode
        0; for a row in mode 1, 1 (MD1) where the packet's sequence number first_seq + seq_base[i] + p is even and 2 (MD2 || HB) where
        it is odd.  streams: position i is row streams[i] (None: row i, n = n_rows); send uint8 [n, n_packets]: the caller's own mask,
        ANDed in; out=: where the mask goes (out=send works in place).  A bad list writes nothing.  Enqueued on the current stream."""
        t = self.torch
        rows = self._rows(streams)
        n, P = self._n(rows), int(n_packets)
        _tensor("mode", mode, t.uint8, (self.n_rows,))
        _tensor("seq_base", seq_base, t.int32, (n,), optional=True)
        _tensor("send", send, t.uint8, (n, P), optional=True)
        _tensor("out", out, t.uint8, (n, P), optional=True)
        first_seq = int(first_seq)
        if P < 1 or n * P >= 2 ** 31 or not -2 ** 31 <= first_seq < 2 ** 31:
            raise ValueError("n_packets >= 1, n * n_packets below 2^31, first_seq inside int32")
        if out is None:
            out = t.zeros((n, P), dtype=t.uint8, device=mode.device)
        r = self.lib.solo_rate_send_mask(mode.data_ptr(), self.n_rows, _ptr(rows), n, P, _ptr(seq_base), first_seq, _ptr(send), out.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_rate_send_mask -> %d" % r)
        return out

    def count(self, count):
        """the count tensor of update() as a dict (synchronises)"""
        return {k: v for k, v in _counts(solo_rate_count_t, count).items() if not k.startswith("reserved")}


class Rtp(_RowObject):
    """An RTP session beside a handle (solo_rtp_*, include/solo_mi355x.h): per stream an SSRC, the random timestamp and sequence
    offsets of RFC 3550 and two payload types; pack() frames the records of send_pack() / send_fanout() for the socket, parse() turns
    received datagrams into the arrivals recv_insert() takes, in place.  The device code has no mutable state."""

    PACK_COUNT = ("dgrams", "dgrams_needed", "bytes", "bytes_needed", "refused")
    PARSE_COUNT = ("accepted", "with_level", "malformed", "version", "unknown_ssrc", "unknown_pt", "timestamp")
    PREFIX = "rtp"

    def __init__(self, n_streams, packet_samples=PACKET_SAMPLES):
        self.n_rows = self.n_streams = int(n_streams)
        self.packet_samples = int(packet_samples)
        self.level_id = 0
        self.trailer = 0
        if self.n_streams <= 0 or self.packet_samples not in (320, 640, 1280):
            raise ValueError("n_streams must be positive, packet_samples 320, 640 or 1280")
        self._create(self.n_streams, self.packet_samples)

    @staticmethod
    def _per_stream(v, n, name, top):
        """a scalar or one value per listed stream, each inside [0, top] -> list"""
        try:
            vals = [int(x) for x in (v.tolist() if hasattr(v, "tolist") else v)] if hasattr(v, "__len__") else [int(v)] * n
        except (TypeError, ValueError):
            vals = None
        if vals is None or len(vals) != n or any(not 0 <= x <= top for x in vals):
            raise ValueError("%s: a scalar or %d values inside [0, %d]" % (name, n, top))
        return vals

    def bind(self, streams, ssrc, ts_offset=0, seq_offset=0, pt=(96, 97), level_id=0):
        """Bind the listed streams (a host sequence inside [0, n_streams), none twice): ssrc (32 bits), ts_offset (32 bits) and seq_offset
        (16 bits) a scalar or one value per listed stream; pt = (MD1's, MD2 || HB's) payload type, 0 .. 127, one pair or one per listed
        stream (equal types: the receiver reads the description from the payload); level_id 0 .. 14, the RFC 8285 id of the audio level
        (0: none), for the whole session: the latest bind wins.  An SSRC that two bound streams would share is refused (RuntimeError), and
        nothing changes.  Ordered on the current stream; synchronises; not capturable."""
        idx = _distinct("streams", streams, self.n_streams)
        n = len(idx)
        ssrc = self._per_stream(ssrc, n, "ssrc", 2 ** 32 - 1)
        ts = self._per_stream(ts_offset, n, "ts_offset", 2 ** 32 - 1)
        sq = self._per_stream(seq_offset, n, "seq_offset", 2 ** 16 - 1)
        try:
            pairs = [tuple(int(x) for x in q) for q in pt] if hasattr(pt[0], "__len__") else [tuple(int(x) for x in pt)] * n
        except (TypeError, ValueError, IndexError):
            pairs = None
        if pairs is None or len(pairs) != n or any(len(q) != 2 or not (0 <= q[0] <= 127 and 0 <= q[1] <= 127) for q in pairs):
            raise ValueError("pt: a pair of payload types inside 0 .. 127, or %d pairs" % n)
        level_id = int(level_id)
        if not 0 <= level_id <= 14:
            raise ValueError("level_id: 0 .. 14")
        self._call("bind", (C.c_int32 * n)(*idx), n, (C.c_uint32 * n)(*ssrc), (C.c_uint32 * n)(*ts), (C.c_uint16 * n)(*sq),
                   (C.c_uint8 * n)(*[q[0] for q in pairs]), (C.c_uint8 * n)(*[q[1] for q in pairs]), level_id)
        self.level_id = level_id

    def unbind(self, streams):
        """Take the binding of the listed streams away: their records are refused by pack(), their datagrams are unknown_ssrc to parse()"""
        idx = _distinct("streams", streams, self.n_streams)
        self._call("unbind", (C.c_int32 * len(idx))(*idx), len(idx))

    def reset(self, rows=None):
        """unbind the listed streams (None: all of them)"""
        self.unbind(range(self.n_streams) if rows is None else rows)

    def pack(self, records, send_count, payload, level=None, dgrams=None, wire=None):
        """records int32 [max,5], send_count int32 [8] and payload uint8 [bytes] as send_pack() / send_fanout() returned them, level uint8
        [n_streams, depth] or None (the byte of packet seq of stream s is level[s, seq % depth]; it needs a level_id) -> (dgrams int32
        [max,2] = (offset, len) of datagram k = record k inside wire, (0, 0) where it is refused or cut; wire uint8 [cap]: 12 (20 with
        levels) header bytes, then the payload, every datagram at a multiple of 4; count int32 [8] on the device, read with pack_count()).
        The number of records is min(send_count's records, max), read on the device.  dgrams / wire: the caller's buffers; the default
        wire, bytes + 23 x max, is never too small for the records of send_pack() (for those of send_fanout(), whose offsets repeat,
        bring one: bytes_needed of the count says how large).  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        m, _ = _tensor("records", records, t.int32, (None, 5))
        _tensor("send_count", send_count, t.int32, (8,))
        nbytes, = _tensor("payload", payload, t.uint8, (None,))
        depth = _tensor("level", level, t.uint8, (self.n_streams, None), optional=True)
        depth = 0 if depth is None else depth[1]
        if m < 1 or (level is not None and (depth < 1 or not self.level_id)):
            raise ValueError("records: at least one; level: a depth of at least 1 and a session with a level_id")
        _tensor("dgrams", dgrams, t.int32, (m, 2), optional=True)
        _tensor("wire", wire, t.uint8, (None,), optional=True)
        if dgrams is None:
            dgrams = t.zeros((m, 2), dtype=t.int32, device=records.device)
        if wire is None:
            wire = t.zeros((nbytes + (23 + getattr(self, "trailer", 0)) * m,), dtype=t.uint8, device=records.device)
        count = t.zeros((8,), dtype=t.int32, device=records.device)
        # (an empty tensor has no address: a cap of 0 only counts, the pointer is never used -- the library still wants one)
        self._call("pack", records.data_ptr(), send_count.data_ptr(), m, payload.data_ptr() or count.data_ptr(), nbytes, _ptr(level), depth,
                   dgrams.data_ptr(), wire.data_ptr() or count.data_ptr(), wire.shape[0], count.data_ptr())
        return dgrams, wire, count

    def parse(self, batch, dgrams, wire, arrivals=None, level=False, rtp_seq=False):
        """dgrams int32 [n,2] = (offset, len) of the received datagrams inside wire uint8 [bytes]; batch: the receiving SoloBatch (with a
        ring, the session's stream count and packet samples) -> (arrivals int32 [n,5] for batch.recv_insert(arrivals, wire): the offsets
        point at the payloads inside wire, a rejected datagram is (-1, 0, 0, 0, 0), which the ring counts as bad; level uint8 [n] or None;
        rtp_seq int16 [n] (the raw 16 bits) or None; count int32 [8] on the device, read with parse_count()).  level / rtp_seq: True = wanted,
        or the caller's tensor.  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        n, _ = _tensor("dgrams", dgrams, t.int32, (None, 2))
        nbytes, = _tensor("wire", wire, t.uint8, (None,))
        _tensor("arrivals", arrivals, t.int32, (n, 5), optional=True)
        if not isinstance(batch, SoloBatch) or batch.n_streams != self.n_streams or batch.packet_samples != self.packet_samples:
            raise ValueError("batch: a SoloBatch of %d streams and %d samples a packet" % (self.n_streams, self.packet_samples))
        outs = []
        for name, x, dtype in (("level", level, t.uint8), ("rtp_seq", rtp_seq, t.int16)):
            if x is True:
                x = t.zeros((n,), dtype=dtype, device=dgrams.device)
            elif x is False or x is None:
                x = None
            else:
                _tensor(name, x, dtype, (n,))
            outs.append(x)
        if arrivals is None:
            arrivals = t.zeros((n, 5), dtype=t.int32, device=dgrams.device)
        count = t.zeros((8,), dtype=t.int32, device=dgrams.device)
        r = self.lib.solo_rtp_parse(self.h, batch.h, dgrams.data_ptr() or count.data_ptr(), n, wire.data_ptr() or count.data_ptr(), nbytes,
                                    arrivals.data_ptr() or count.data_ptr(), _ptr(outs[0]), _ptr(outs[1]), count.data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_rtp_parse -> %d" % r)
        return arrivals, outs[0], outs[1], count

    # ---- SRTP (solo_srtp_*): keys per stream, protect() behind pack(), unprotect() in front of parse() ----
    def set_trailer(self, trailer_bytes):
        """bytes pack() keeps free (and zero) behind every datagram: the room of the SRTP tag, 0 .. 16; dgrams[k].len stays the RTP
        packet's, the offsets and byte counts include the trailer.  Read by the next pack()."""
        trailer_bytes = int(trailer_bytes)
        if not 0 <= trailer_bytes <= 16:
            raise ValueError("trailer_bytes: 0 .. 16")
        r = self.lib.solo_rtp_set_trailer(self.h, trailer_bytes)
        if r:
            raise RuntimeError("solo_rtp_set_trailer -> %d" % r)
        self.trailer = trailer_bytes

    @staticmethod
    def _masters(name, v, n, each=SRTP_MASTER_BYTES):
        """None, or n x `each` bytes of keying material (bytes, a sequence of bytes objects, or a uint8 array [n,each]) -> ctypes array"""
        if v is None:
            return None
        try:
            raw = bytes(v) if isinstance(v, (bytes, bytearray)) else v.tobytes() if hasattr(v, "tobytes") else b"".join(bytes(x) for x in v)
        except (TypeError, ValueError):
            raw = b""
        if len(raw) != each * n:
            raise ValueError("%s: %d x %d bytes (master key || master salt per listed stream) or None" % (name, n, each))
        return (C.c_uint8 * len(raw)).from_buffer_copy(raw)

    def set_keys(self, streams, tx=None, rx=None, rx_roc=None, tag_bytes=10):
        """SRTP keys of the listed streams (a host sequence inside [0, n_streams), none twice): tx / rx = 30 bytes of keying material per
        listed stream (master key || master salt, as SDES or DTLS-SRTP give them) or None = that direction keeps what it had; rx_roc: the
        receiver's initial rollover counter, a scalar or one per listed stream; tag_bytes 10 or 4.  A tx key needs a trailer of at least
        tag_bytes (set_trailer).  Setting an rx key resets the stream's receive index.  Ordered on the current stream; synchronises; not
        capturable."""
        idx = _distinct("streams", streams, self.n_streams)
        n = len(idx)
        txa, rxa = self._masters("tx", tx, n), self._masters("rx", rx, n)
        tag_bytes = int(tag_bytes)
        if tag_bytes not in (4, 10) or (txa is None and rxa is None):
            raise ValueError("tag_bytes: 10 or 4; at least one of tx and rx")
        if txa is not None and self.trailer < tag_bytes:
            raise ValueError("a tx key needs set_trailer(%d) or more first" % tag_bytes)
        roc = None if rx_roc is None else (C.c_uint32 * n)(*self._per_stream(rx_roc, n, "rx_roc", 2 ** 32 - 1))
        self._call("set_keys", (C.c_int32 * n)(*idx), n, txa, rxa, roc, tag_bytes, prefix="srtp")

    def set_keys_gcm(self, streams, tx=None, rx=None, rx_roc=None):
        """set_keys() for AEAD_AES_128_GCM (RFC 7714): tx / rx = 28 bytes of keying material per listed stream (master key || 12-byte
        master salt, as DTLS-SRTP gives them for SRTP_AEAD_AES_128_GCM); the tag is always 16 bytes, so a tx key needs set_trailer(16).
        A stream and direction has one key: the last set call wins, whichever transform it names."""
        idx = _distinct("streams", streams, self.n_streams)
        n = len(idx)
        txa, rxa = self._masters("tx", tx, n, SRTP_GCM_MASTER_BYTES), self._masters("rx", rx, n, SRTP_GCM_MASTER_BYTES)
        if txa is None and rxa is None:
            raise ValueError("at least one of tx and rx")
        if txa is not None and self.trailer < SRTP_GCM_TAG_BYTES:
            raise ValueError("a tx key needs set_trailer(%d) first" % SRTP_GCM_TAG_BYTES)
        roc = None if rx_roc is None else (C.c_uint32 * n)(*self._per_stream(rx_roc, n, "rx_roc", 2 ** 32 - 1))
        self._call("set_keys_gcm", (C.c_int32 * n)(*idx), n, txa, rxa, roc, prefix="srtp")

    def clear_keys(self, streams):
        """both keys and the receive index of the listed streams go; unbind() does the same"""
        idx = _distinct("streams", streams, self.n_streams)
        self._call("clear_keys", (C.c_int32 * len(idx))(*idx), len(idx), prefix="srtp")

    def rx_index(self, streams=None):
        """the highest authenticated packet index (ROC << 16 | SEQ) of the listed streams (None: all), -1 = none yet (synchronises)"""
        idx = list(range(self.n_streams)) if streams is None else _distinct("streams", streams, self.n_streams)
        out = (C.c_int64 * len(idx))()
        self._call("get_rx_index", (C.c_int32 * len(idx))(*idx), len(idx), out, prefix="srtp")
        return list(out)

    def protect(self, records, send_count, dgrams, wire):
        """behind pack(records, send_count, ...) -> (dgrams, wire, count): the datagrams of pack() become SRTP in place (the payload
        encrypted, the tag in the trailer, dgrams[k].len grown by the tag); a datagram of a stream without a tx key becomes (0, 0) and is
        counted no_key -> count int32 [8] on the device, read with srtp_count().  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        m, _ = _tensor("records", records, t.int32, (None, 5))
        _tensor("send_count", send_count, t.int32, (8,))
        _tensor("dgrams", dgrams, t.int32, (m, 2))
        nbytes, = _tensor("wire", wire, t.uint8, (None,))
        if m < 1:
            raise ValueError("records: at least one")
        count = t.zeros((8,), dtype=t.int32, device=records.device)
        self._call("protect", records.data_ptr(), send_count.data_ptr(), m, dgrams.data_ptr(), wire.data_ptr() or count.data_ptr(), nbytes, count.data_ptr(),
                   prefix="srtp")
        return count

    def unprotect(self, dgrams, wire, dgrams_out=None):
        """in front of parse(): dgrams int32 [n,2] of received SRTP datagrams inside wire -> (dgrams_out int32 [n,2] for parse(): the RTP
        packet of an accepted datagram, decrypted in place, (0, 0) for a rejected one, whose bytes stay as they were; count int32 [8] on
        the device, read with srtp_count()).  dgrams_out may be dgrams.  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        n, _ = _tensor("dgrams", dgrams, t.int32, (None, 2))
        nbytes, = _tensor("wire", wire, t.uint8, (None,))
        _tensor("dgrams_out", dgrams_out, t.int32, (n, 2), optional=True)
        if dgrams_out is None:
            dgrams_out = t.zeros((n, 2), dtype=t.int32, device=dgrams.device)
        count = t.zeros((8,), dtype=t.int32, device=dgrams.device)
        self._call("unprotect", dgrams.data_ptr() or count.data_ptr(), n, wire.data_ptr() or count.data_ptr(), nbytes,
                   dgrams_out.data_ptr() or count.data_ptr(), count.data_ptr(), prefix="srtp")
        return dgrams_out, count

    def srtp_count(self, count):
        """the count tensor of protect() / unprotect() as a dict (synchronises); ok == -1: the list behind protect's records was refused"""
        return _counts(solo_srtp_count_t, count)

    # ---- SRTCP (solo_srtcp_*): RTCP keys and indices per stream, protect_rtcp() behind Rtcp.build(), unprotect_rtcp() in front of Rtcp.parse() ----
    def set_rtcp_keys(self, streams, tx=None, rx=None, tx_index=None, rx_index=None):
        """SRTCP keys of the listed streams (a host sequence inside [0, n_streams), none twice): tx / rx = 30 bytes of keying material per
        listed stream (master key || master salt) or None = that direction keeps what it had; tx_index: the index the next protected
        packet gets, 0 .. 2^31, a scalar or one per listed stream (None: 0); rx_index: the highest index already authenticated, -1 ..
        2^31 - 1, likewise (None: -1, none yet).  The tag is always 10 bytes.  Ordered on the current stream; synchronises; not
        capturable."""
        idx = _distinct("streams", streams, self.n_streams)
        n = len(idx)
        txa, rxa = self._masters("tx", tx, n), self._masters("rx", rx, n)
        if txa is None and rxa is None:
            raise ValueError("at least one of tx and rx")
        ti = None if tx_index is None else (C.c_uint32 * n)(*self._per_stream(tx_index, n, "tx_index", 2 ** 31))
        ri = None if rx_index is None else (C.c_int64 * n)(*[v - 1 for v in self._per_stream(self._plus_one(rx_index), n, "rx_index + 1", 2 ** 31)])
        self._call("set_keys", (C.c_int32 * n)(*idx), n, txa, rxa, ti, ri, prefix="srtcp")

    def set_rtcp_keys_gcm(self, streams, tx=None, rx=None, tx_index=None, rx_index=None):
        """set_rtcp_keys() for AEAD_AES_128_GCM (RFC 7714): tx / rx = 28 bytes of keying material per listed stream (master key || 12-byte
        master salt).  The trailer of such a stream's packets is 20 bytes (the 16-byte tag, then E || index): protect_rtcp() needs
        rtcp.set_trailer(20) while the session holds a GCM tx key."""
        idx = _distinct("streams", streams, self.n_streams)
        n = len(idx)
        txa, rxa = self._masters("tx", tx, n, SRTP_GCM_MASTER_BYTES), self._masters("rx", rx, n, SRTP_GCM_MASTER_BYTES)
        if txa is None and rxa is None:
            raise ValueError("at least one of tx and rx")
        ti = None if tx_index is None else (C.c_uint32 * n)(*self._per_stream(tx_index, n, "tx_index", 2 ** 31))
        ri = None if rx_index is None else (C.c_int64 * n)(*[v - 1 for v in self._per_stream(self._plus_one(rx_index), n, "rx_index + 1", 2 ** 31)])
        self._call("set_keys_gcm", (C.c_int32 * n)(*idx), n, txa, rxa, ti, ri, prefix="srtcp")

    @staticmethod
    def _plus_one(v):
        """rx_index (-1 = none yet) moved to 0 .. 2^31 for the range check of _per_stream; what is no integer goes through and is refused there"""
        try:
            return [int(x) + 1 for x in (v.tolist() if hasattr(v, "tolist") else v)] if hasattr(v, "__len__") else int(v) + 1
        except (TypeError, ValueError):
            return None

    def clear_rtcp_keys(self, streams):
        """both SRTCP keys, the send index and the receive index of the listed streams go; unbind() does the same"""
        idx = _distinct("streams", streams, self.n_streams)
        self._call("clear_keys", (C.c_int32 * len(idx))(*idx), len(idx), prefix="srtcp")

    def rtcp_index(self, streams=None):
        """(tx_next, rx_index) of the listed streams (None: all): the index the next protected packet gets, and the highest authenticated
        one, -1 = none yet (synchronises).  With set_rtcp_keys(tx_index=, rx_index=) the hand-over to another session."""
        idx = list(range(self.n_streams)) if streams is None else _distinct("streams", streams, self.n_streams)
        tx, rx = (C.c_uint32 * len(idx))(), (C.c_int64 * len(idx))()
        self._call("get_index", (C.c_int32 * len(idx))(*idx), len(idx), tx, rx, prefix="srtcp")
        return list(tx), list(rx)

    def protect_rtcp(self, rtcp, streams, build_count, dgrams, wire):
        """behind rtcp.build(self, ..., streams, ...) -> (dgrams, wire, build_count) with rtcp.set_trailer(14) or more: the compound
        packets become SRTCP in place (bytes from 8 on encrypted, E || index and the tag in the trailer, dgrams[i].len grown by 14, the
        stream's send index advanced); a packet of a stream without a tx key, or whose key is used up, becomes (0, 0).  streams: the int32
        CUDA tensor [n] the build call had -> count int32 [8] on the device, read with srtcp_count().  Enqueued on the current stream,
        no synchronisation."""
        t = self.torch
        if not isinstance(rtcp, Rtcp) or rtcp.n_streams != self.n_streams or not rtcp.h:
            raise ValueError("rtcp: an Rtcp object of %d streams" % self.n_streams)
        if rtcp.trailer < SRTCP_TRAILER_BYTES:
            raise ValueError("rtcp: set_trailer(%d) or more before the build call" % SRTCP_TRAILER_BYTES)
        n, = _tensor("streams", streams, t.int32, (None,))
        if not 0 < n <= self.n_streams:
            raise ValueError("streams: 1 .. %d indices" % self.n_streams)
        _tensor("build_count", build_count, t.int32, (8,))
        _tensor("dgrams", dgrams, t.int32, (n, 2))
        nbytes, = _tensor("wire", wire, t.uint8, (None,))
        count = t.zeros((8,), dtype=t.int32, device=dgrams.device)
        r = self.lib.solo_srtcp_protect(rtcp.h, self.h, streams.data_ptr(), n, build_count.data_ptr(), dgrams.data_ptr(), wire.data_ptr() or count.data_ptr(),
                                        nbytes, count.data_ptr(), self._stream())
        if r == -1 and rtcp.trailer < SRTCP_GCM_TRAILER_BYTES:
            # every other refusal of the call is checked above: the library, which alone knows the session's keys, holds a GCM tx key
            raise ValueError("rtcp: set_trailer(%d) before the build call: the session holds a GCM tx key" % SRTCP_GCM_TRAILER_BYTES)
        if r:
            raise RuntimeError("solo_srtcp_protect -> %d" % r)
        return count

    def unprotect_rtcp(self, dgrams, wire, dgrams_out=None):
        """in front of Rtcp.parse(self, ...): dgrams int32 [n,2] of received SRTCP datagrams inside wire -> (dgrams_out int32 [n,2] for
        parse(): the compound packet of an accepted datagram, decrypted in place, (0, 0) for a rejected one, whose bytes stay as they
        were; count int32 [8] on the device, read with srtcp_count()).  A datagram is accepted only if its index is newer than everything
        authenticated for its stream before this call.  dgrams_out may be dgrams.  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        n, _ = _tensor("dgrams", dgrams, t.int32, (None, 2))
        nbytes, = _tensor("wire", wire, t.uint8, (None,))
        _tensor("dgrams_out", dgrams_out, t.int32, (n, 2), optional=True)
        if dgrams_out is None:
            dgrams_out = t.zeros((n, 2), dtype=t.int32, device=dgrams.device)
        count = t.zeros((8,), dtype=t.int32, device=dgrams.device)
        self._call("unprotect", dgrams.data_ptr() or count.data_ptr(), n, wire.data_ptr() or count.data_ptr(), nbytes,
                   dgrams_out.data_ptr() or count.data_ptr(), count.data_ptr(), prefix="srtcp")
        return dgrams_out, count

    def srtcp_count(self, count):
        """the count tensor of protect_rtcp() / unprotect_rtcp() as a dict (synchronises); ok == -1: the list behind the build was refused"""
        return _counts(solo_srtcp_count_t, count)

    def pack_count(self, count):
        """the count tensor of pack() as a dict (synchronises); dgrams == -1: the list behind the records was refused on the device"""
        return _counts(solo_rtp_pack_count_t, count)

    def parse_count(self, count):
        """the count tensor of parse() as a dict (synchronises): datagrams per verdict"""
        return _counts(solo_rtp_parse_count_t, count)

    def close(self):
        if getattr(self, "h", None):
            self.lib.solo_rtp_destroy(self.h)
            self.h = None


FORWARD_MAX_SLOTS = 8


class Forward(_RowStateObject):
    """The middle of a forwarding server's tick (solo_forward_*, include/solo_mi355x.h): levels() turns the arrivals Rtp.parse() wrote into
    one RFC 6464 level per row for Vad.select(), route() turns the selected speakers' arrivals into records for the egress Rtp.pack()
    -- one per other member of the sender's room, under `slots` per-room slots whose packet numbers stay continuous when the speaker
    behind a slot changes.  Nothing is decoded and no payload byte moves.  The state is 16 bytes per ROOM and slot: a "row" of this
    object is a room."""

    COUNT = ("forwarded", "rejected", "no_desc", "no_room", "not_selected", "no_slot", "stale", "switches")
    PREFIX = "forward"

    def __init__(self, n_rows, slots=3):
        self.n_rows, self.slots = int(n_rows), int(slots)
        if self.n_rows <= 0 or not 1 <= self.slots <= FORWARD_MAX_SLOTS:
            raise ValueError("n_rows must be positive, slots 1 .. %d" % FORWARD_MAX_SLOTS)
        self.state_bytes = 16 * self.slots
        self._create(self.n_rows, self.slots)

    def levels(self, arrivals, level_in=None, default_level=255, n_rows=None):
        """arrivals int32 [n_dgrams,5] and level_in uint8 [n_dgrams] (or None: every datagram has default_level) as Rtp.parse() wrote
        them; default_level 0 .. 255: the byte of a datagram that carries none (255: it has none) -> dict(rowinfo int32 [n_rows,4] =
        solo_forward_row_t per row, what route() takes; sa uint8 [n_rows] and level uint8 [n_rows]: what Vad.select() takes as sa[:, None,
        None] and level[:, None]).  Stateless.  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        nd, _ = _tensor("arrivals", arrivals, t.int32, (None, 5))
        _tensor("level_in", level_in, t.uint8, (nd,), optional=True)
        n_rows, default_level = self.n_rows if n_rows is None else int(n_rows), int(default_level)
        if n_rows <= 0 or not 0 <= default_level <= 255:
            raise ValueError("n_rows must be positive, default_level 0 .. 255")
        out = {"rowinfo": t.zeros((n_rows, 4), dtype=t.int32, device=arrivals.device), "sa": t.zeros((n_rows,), dtype=t.uint8, device=arrivals.device),
               "level": t.zeros((n_rows,), dtype=t.uint8, device=arrivals.device)}
        r = self.lib.solo_forward_levels(arrivals.data_ptr() or None, _ptr(level_in) or None, nd, n_rows, default_level, out["rowinfo"].data_ptr(),
                                         out["sa"].data_ptr(), out["level"].data_ptr(), self._stream())
        if r:
            raise RuntimeError("solo_forward_levels -> %d" % r)
        return out

    def route(self, arrivals, rowinfo, sel, room, n_rooms=None, max_records=None, records=None):
        """arrivals int32 [n_dgrams,5]; rowinfo int32 [n,4] as levels() wrote it; sel uint8 [n] (or [n,1]) as Vad.select() wrote it for one
        packet; room int32 [n] (-1 = in no room; n_rooms=None: the largest id + 1, which synchronises) -> dict(records int32 [max,5] for the
        egress Rtp.pack(records, send_count, the receive buffer, level=level_fwd): stream = receiver x slots + slot; send_count int32 [8];
        level_fwd uint8 [n x slots, 1]; slot_src int32 [n_rooms, slots]: the row each slot carries, -1 = free; count int32 [8], read with
        count()).  max_records=None: n_dgrams x (n - 1), never too small; records: the caller's buffer.  A room id outside [-1, n_rooms) is
        refused on the device: forwarded == -1 in the count, records == -1 in send_count, nothing else written.  Enqueued on the
        current stream; synchronises only when a call has more datagrams than every one before it."""
        t = self.torch
        nd, _ = _tensor("arrivals", arrivals, t.int32, (None, 5))
        n, _ = _tensor("rowinfo", rowinfo, t.int32, (None, 4))
        if not 0 < n <= self.n_rows:
            raise ValueError("rowinfo: 1 .. %d rows" % self.n_rows)
        if getattr(sel, "dim", None) and sel.dim() == 2:
            _tensor("sel", sel, t.uint8, (n, 1))
        else:
            _tensor("sel", sel, t.uint8, (n,))
        _tensor("room", room, t.int32, (n,))
        if n_rooms is None:
            n_rooms = max(int(room.max()) + 1, 1)
        n_rooms = int(n_rooms)
        if not 0 < n_rooms <= self.n_rows:
            raise ValueError("n_rooms: 1 .. %d" % self.n_rows)
        if nd * (n - 1) >= 2 ** 31:
            raise ValueError("n_dgrams x (n - 1) must stay below 2^31")
        if records is not None:
            max_records, _ = _tensor("records", records, t.int32, (None, 5))
        max_records = nd * (n - 1) if max_records is None else int(max_records)
        if max_records < 0:
            raise ValueError("max_records: not negative")
        dev = rowinfo.device
        if records is None:
            records = t.zeros((max(max_records, 1), 5), dtype=t.int32, device=dev)
        out = {"records": records, "send_count": t.zeros((8,), dtype=t.int32, device=dev),
               "level_fwd": t.full((n * self.slots, 1), 0x7F, dtype=t.uint8, device=dev),
               "slot_src": t.full((n_rooms, self.slots), -1, dtype=t.int32, device=dev), "count": t.zeros((8,), dtype=t.int32, device=dev)}
        self._call("route", arrivals.data_ptr() or None, nd, rowinfo.data_ptr(), sel.data_ptr(), room.data_ptr(), n, n_rooms, records.data_ptr(), max_records,
                   out["send_count"].data_ptr(), out["level_fwd"].data_ptr(), out["slot_src"].data_ptr(), out["count"].data_ptr())
        return out

    def count(self, count):
        """the count tensor of route() as a dict (synchronises); forwarded == -1: the call was refused on the device"""
        return _counts(solo_forward_count_t, count)

    def reset(self, rooms=None):
        """every room, or the listed rooms (a host sequence: inside [0, n_rows), none twice), back to free slots that start at packet 0"""
        if rooms is None:
            return self._call("reset")
        idx = _distinct("rooms", rooms, self.n_rows)
        self._call("reset_rooms", (C.c_int32 * len(idx))(*idx), len(idx))

    def close(self):
        if getattr(self, "h", None):
            self.lib.solo_forward_destroy(self.h)
            self.h = None


RTCP_STATE_BYTES = 128
RTCP_CNAME_BYTES = 32
RTCP_WALK_MAX = 128
RTCP_BYE = 1 << 30


class Rtcp(_RowStateObject):
    """RTCP beside the Rtp sessions of n_streams streams (solo_rtcp_*, include/solo_mi355x.h): received() keeps the reception statistics
    of RFC 3550 A.1 / A.8 from the arrivals Rtp.parse() wrote, sent() the sender's counts from what Rtp.pack() / protect() left, build()
    writes one compound SR / RR + SDES packet per listed stream and parse() turns the peers' packets into round-trip time and loss
    feedback.  The state is 128 bytes a row; a state blob carries the row's CNAME (32 bytes) behind them."""

    COUNT = {"received": solo_rtcp_received_count_t, "sent": solo_rtcp_sent_count_t, "build": solo_rtcp_build_count_t, "parse": solo_rtcp_parse_count_t}
    PREFIX = "rtcp"
    state_bytes = RTCP_STATE_BYTES + RTCP_CNAME_BYTES

    def __init__(self, n_streams):
        self.n_rows = self.n_streams = int(n_streams)
        self.trailer = 0
        if self.n_streams <= 0:
            raise ValueError("n_streams must be positive")
        self._create(self.n_streams)

    def set_trailer(self, trailer_bytes):
        """bytes build() keeps free (and zero) behind every packet: the room of the SRTCP trailer (Rtp.protect_rtcp() needs 14, and 20
        with GCM keys), 0 .. 16 or 20; dgrams[i].len stays the compound packet's, the offsets and byte counts include the trailer.
        Read by the next build()."""
        trailer_bytes = int(trailer_bytes)
        if not 0 <= trailer_bytes <= 16 and trailer_bytes != SRTCP_GCM_TRAILER_BYTES:
            raise ValueError("trailer_bytes: 0 .. 16, or 20")
        r = self.lib.solo_rtcp_set_trailer(self.h, trailer_bytes)
        if r:
            raise RuntimeError("solo_rtcp_set_trailer -> %d" % r)
        self.trailer = trailer_bytes

    def _session(self, name, r, optional=False):
        if r is None and optional:
            return None
        if not isinstance(r, Rtp) or r.n_streams != self.n_streams or not r.h:
            raise ValueError("%s: an Rtp session of %d streams%s" % (name, self.n_streams, " or None" if optional else ""))
        return r.h

    def _now(self, now_ntp):
        """the time of a build() / parse() call: an int (64 bits, 32.32) or a CUDA int64 tensor [1] -> (scalar, pointer)"""
        if getattr(now_ntp, "is_cuda", False):
            _tensor("now_ntp", now_ntp, self.torch.int64, (1,))
            return 0, now_ntp.data_ptr()
        now_ntp = int(now_ntp)
        if not 0 <= now_ntp < 2 ** 64:
            raise ValueError("now_ntp: 0 .. 2^64 - 1, or an int64 CUDA tensor [1]")
        return now_ntp, None

    def set_cname(self, streams, names):
        """the CNAME of the listed streams (a host sequence inside [0, n_streams), none twice): one str / bytes of 1 .. 31 bytes, or one per
        listed stream.  Ordered on the current stream; synchronises; not capturable."""
        idx = _distinct("streams", streams, self.n_streams)
        if isinstance(names, (str, bytes)):
            names = [names] * len(idx)
        raw = [x.encode("utf-8") if isinstance(x, str) else bytes(x) for x in names]
        if len(raw) != len(idx) or any(not 1 <= len(x) <= RTCP_CNAME_BYTES - 1 or 0 in x for x in raw):
            raise ValueError("names: one name of 1 .. %d bytes without a zero byte, or %d of them" % (RTCP_CNAME_BYTES - 1, len(idx)))
        buf = b"".join(x.ljust(RTCP_CNAME_BYTES, b"\0") for x in raw)
        self._call("set_cname", (C.c_int32 * len(idx))(*idx), len(idx), buf)

    def received(self, rtp, arrivals, rtp_seq, arrival_time=None, now_rtp=0):
        """behind rtp.parse(..., rtp_seq=True): arrivals int32 [n,5] and rtp_seq int16 [n] as it wrote them; arrival_time int32 [n] (the 32
        bits of the caller's clock in RTP timestamp units) or None = every datagram arrived at now_rtp -> count int32 [8] on the device,
        read with count("received", c).  Enqueued on the current stream; synchronises only when a call has more datagrams than every
        one before it."""
        t = self.torch
        n, _ = _tensor("arrivals", arrivals, t.int32, (None, 5))
        _tensor("rtp_seq", rtp_seq, t.int16, (n,))
        _tensor("arrival_time", arrival_time, t.int32, (n,), optional=True)
        now_rtp = int(now_rtp)
        if not 0 <= now_rtp < 2 ** 32:
            raise ValueError("now_rtp: 0 .. 2^32 - 1")
        count = t.zeros((8,), dtype=t.int32, device=arrivals.device)
        self._call("received", self._session("rtp", rtp), arrivals.data_ptr() or None, rtp_seq.data_ptr() or None, n, _ptr(arrival_time) or None, now_rtp,
                   count.data_ptr())
        return count

    def sent(self, rtp, records, send_count, dgrams):
        """behind rtp.pack() or rtp.protect(): records int32 [max,5], send_count int32 [8] and dgrams int32 [max,2] as they left them ->
        count int32 [8] on the device, read with count("sent", c).  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        m, _ = _tensor("records", records, t.int32, (None, 5))
        _tensor("send_count", send_count, t.int32, (8,))
        _tensor("dgrams", dgrams, t.int32, (m, 2))
        if m < 1:
            raise ValueError("records: at least one")
        count = t.zeros((8,), dtype=t.int32, device=records.device)
        self._call("sent", self._session("rtp", rtp), records.data_ptr(), send_count.data_ptr(), m, dgrams.data_ptr(), count.data_ptr())
        return count

    def build(self, rtp_tx, rtp_rx, streams, now_ntp, dgrams=None, wire=None):
        """one compound packet (SR or RR, with a report block where rtp_rx is given and the stream has received, then SDES CNAME) per listed
        stream: streams a strictly increasing host sequence or an int32 CUDA tensor [n]; now_ntp an int (32.32) or an int64 CUDA tensor
        [1], which a captured call reads at every replay -> (dgrams int32 [n,2], wire uint8 [cap], count int32 [8], read with
        count("build", c)).  The default wire, 96 bytes a packet and the trailer of set_trailer(), is never too small.  Enqueued on the current stream, no synchronisation."""
        t = self.torch
        rows = self._rows(streams)
        if rows is None:
            raise ValueError("streams: a list")
        n = int(rows.shape[0])
        now, d_now = self._now(now_ntp)
        _tensor("dgrams", dgrams, t.int32, (n, 2), optional=True)
        _tensor("wire", wire, t.uint8, (None,), optional=True)
        if dgrams is None:
            dgrams = t.zeros((n, 2), dtype=t.int32, device=self.device)
        if wire is None:
            wire = t.zeros(((96 + 4 * ((getattr(self, "trailer", 0) + 3) // 4)) * n,), dtype=t.uint8, device=self.device)
        count = t.zeros((8,), dtype=t.int32, device=self.device)
        self._call("build", self._session("rtp_tx", rtp_tx), self._session("rtp_rx", rtp_rx, optional=True), rows.data_ptr(), n, now, d_now, dgrams.data_ptr(),
                   wire.data_ptr() or count.data_ptr(), wire.shape[0], count.data_ptr())
        return dgrams, wire, count

    def parse(self, rtp_rx, rtp_tx, dgrams, wire, now_ntp, feedback=None):
        """dgrams int32 [n,2] = (offset, len) of received compound packets inside wire uint8 [bytes]; rtp_rx: the session with the peers'
        SSRCs, rtp_tx (or None): ours -> (feedback int32 [n_streams,8] = solo_rtcp_feedback_t per stream, count int32 [16], read with
        count("parse", c)).  Enqueued on the current stream; synchronises only when a call has more datagrams than every one before it."""
        t = self.torch
        n, _ = _tensor("dgrams", dgrams, t.int32, (None, 2))
        nbytes, = _tensor("wire", wire, t.uint8, (None,))
        _tensor("feedback", feedback, t.int32, (self.n_streams, 8), optional=True)
        now, d_now = self._now(now_ntp)
        if feedback is None:
            feedback = t.zeros((self.n_streams, 8), dtype=t.int32, device=self.device)
        count = t.zeros((16,), dtype=t.int32, device=self.device)
        self._call("parse", self._session("rtp_rx", rtp_rx), self._session("rtp_tx", rtp_tx, optional=True), dgrams.data_ptr() or None, n,
                   wire.data_ptr() or None, nbytes, now, d_now, feedback.data_ptr(), count.data_ptr())
        return feedback, count

    def count(self, which, count):
        """the count tensor of received() / sent() / build() / parse() as a dict (synchronises)"""
        if which not in self.COUNT:
            raise ValueError("which: one of %s" % ", ".join(sorted(self.COUNT)))
        return {k: v for k, v in _counts(self.COUNT[which], count).items() if not k.startswith("reserved")}

    def close(self):
        if getattr(self, "h", None):
            self.lib.solo_rtcp_destroy(self.h)
            self.h = None
