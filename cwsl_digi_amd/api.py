"""ctypes mirror of include/cwsl_gpu.h.

Naming follows the reference's seams (source/Receiver.hpp, source/Instance.cpp, source/SSBD.hpp):
a Context owns Receivers (IQ rings in HBM) and Channels (one SSBD + frame pair each); slot
boundaries are signalled per SyncPredicates group.  Every call goes through libcwslgpu.so; if the
library or a gfx950 device is missing this raises -- nothing here computes DSP on the CPU.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))
# CWSLG_LIB: another build of the library -- a path, or "lab" for lib/libcwslgpu_lab.so (the measured alternative kernels and the
# environment switches that select them; the product library has neither)
_LIB_PATH = os.environ.get("CWSLG_LIB") or os.path.join(_HERE, "lib", "libcwslgpu.so")
if _LIB_PATH == "lab":
    _LIB_PATH = os.path.join(_HERE, "lib", "libcwslgpu_lab.so")

STATUS_NAMES = {
    0: "OK", -1: "ERR_RATIO", -2: "ERR_BAND_LOW", -3: "ERR_BAND_HIGH", -4: "ERR_NOMEM", -5: "ERR_MODE",
    -6: "ERR_ARG", -7: "ERR_NO_DEVICE", -8: "ERR_HIP", -9: "ERR_NO_FRAME", -10: "ERR_UNSUPPORTED",
    -11: "ERR_BLOCK",
}
ERR_NO_FRAME = -9
ERR_HIP = -8

# CWSL_DIGI_Types.hpp:83-143
GROUPS = {"FT8": 0, "FT4": 1, "Q65_30": 2, "S60": 3, "S120": 4, "S300": 5, "S900": 6, "S1800": 7}
_MODE_GROUP = {
    "FT8": 0, "JS8": 0, "FT4": 1, "Q65-30": 2, "JT65": 3, "FST4-60": 3, "WSPR": 4, "FST4-120": 4,
    "FST4W-120": 4, "FST4-300": 5, "FST4W-300": 5, "FST4-900": 6, "FST4W-900": 6, "FST4-1800": 7,
    "FST4W-1800": 7,
}
_MODE_PERIOD = {
    "FT8": 15.0, "JS8": 15.0, "FT4": 7.5, "WSPR": 120.0, "Q65-30": 30.0, "JT65": 60.0, "FST4-60": 60.0,
    "FST4-120": 120.0, "FST4-300": 300.0, "FST4-900": 900.0, "FST4-1800": 1800.0, "FST4W-120": 120.0,
    "FST4W-300": 300.0, "FST4W-900": 900.0, "FST4W-1800": 1800.0,
}


def group_of(mode):
    return _MODE_GROUP[mode]


def frame_len(mode):
    """Instance.cpp:149 : 12000 * (period + 5)."""
    return int(12000.0 * float(np.float32(_MODE_PERIOD[mode]) + np.float32(5)))


class CwslGpuError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        name = STATUS_NAMES.get(status, str(status))
        super().__init__(f"libcwslgpu: {name}" + (f": {detail}" if detail else ""))


class DecoderSpec(C.Structure):
    _fields_ = [("freq_hz", C.c_uint32), ("calibrated_hz", C.c_uint32), ("mode", C.c_char * 16), ("smnum", C.c_int32),
                ("freqcal", C.c_double), ("callsign", C.c_char * 16), ("group", C.c_int32),
                ("frame_len", C.c_uint32), ("period_s", C.c_float)]


def parse_decoder_line(line, freqcal_global=1.0):
    """config.ini `decoder=` value -> dict (CWSL_DIGI.cpp:731-837).  Raises CwslGpuError on the reference's error cases."""
    L = load_library()
    sp = DecoderSpec()
    rc = L.cwslg_parse_decoder_line(line.encode(), float(freqcal_global), C.byref(sp))
    if rc != 0:
        raise CwslGpuError(rc, "Error parsing decoder line: " + line)
    return dict(freq_hz=sp.freq_hz, calibrated_hz=sp.calibrated_hz, mode=sp.mode.decode(), smnum=sp.smnum,
                freqcal=sp.freqcal, callsign=sp.callsign.decode(), group=sp.group, frame_len=sp.frame_len,
                period_s=sp.period_s)


class Candidate(C.Structure):
    _fields_ = [("freq_bin", C.c_int32), ("time_step", C.c_int32), ("sync", C.c_float),
                ("freq_hz", C.c_float), ("dt_s", C.c_float)]


class Spot(C.Structure):
    _fields_ = [("snr_db", C.c_int32), ("dt_s", C.c_float), ("freq_hz", C.c_uint32), ("has_locator", C.c_int32),
                ("call", C.c_char * 16), ("locator", C.c_char * 8), ("message", C.c_char * 64), ("drift", C.c_int32), ("dbm", C.c_int32)]


class Ft4Sync(C.Structure):
    _fields_ = [("f0_hz", C.c_float), ("f1_hz", C.c_float), ("dt_s", C.c_float), ("sync", C.c_float),
                ("ibest", C.c_int32), ("idf", C.c_int32), ("seg", C.c_int32), ("cand", C.c_int32)]


class Ft8Soft(C.Structure):
    _fields_ = [("llr", C.c_float * 174), ("sigma", C.c_float), ("nsync", C.c_int32)]


class Ft8Msg(C.Structure):
    _fields_ = [("bits", C.c_uint8 * 12), ("iters", C.c_int16), ("nbad", C.c_int16), ("nharderr", C.c_int16), ("crc_ok", C.c_uint8), ("pad_", C.c_uint8)]


# numpy view of cwslg_ft8_msg (20 bytes)
FT8_MSG_DTYPE = np.dtype([("bits", np.uint8, 12), ("iters", np.int16), ("nbad", np.int16), ("nharderr", np.int16), ("crc_ok", np.uint8), ("pad_", np.uint8)])


class Ft4Msg(C.Structure):
    _fields_ = [("set", Ft8Msg * 3)]


# numpy view of cwslg_ft4_msg (60 bytes): three FT8_MSG_DTYPE records -- rec["set"]["crc_ok"][q, s] is set s of record q
FT4_MSG_DTYPE = np.dtype([("set", FT8_MSG_DTYPE, 3)])


def ft4_best_set(rec):
    """The set a consumer takes from FT4 decode records (FT4_MSG_DTYPE): upstream tries the metric sets in order and stops at the first success,
    which is the smallest s with crc_ok; -1 if none.  One record -> int, an array of records -> int array."""
    ok = np.asarray(rec["set"]["crc_ok"]) != 0
    best = np.where(ok.any(axis=-1), ok.argmax(axis=-1), -1)
    return int(best) if best.ndim == 0 else best.astype(np.int64)


class OsdMsg(C.Structure):
    _fields_ = [("bits", C.c_uint8 * 12), ("dmin", C.c_float), ("nharderr", C.c_int16), ("nskip", C.c_int16), ("crc_ok", C.c_uint8), ("how", C.c_uint8),
                ("flip", C.c_uint8 * 2)]


# numpy view of cwslg_osd_msg (24 bytes)
OSD_MSG_DTYPE = np.dtype([("bits", np.uint8, 12), ("dmin", np.float32), ("nharderr", np.int16), ("nskip", np.int16), ("crc_ok", np.uint8), ("how", np.uint8),
                          ("flip", np.uint8, 2)])


class Ft4Osd(C.Structure):
    _fields_ = [("set", OsdMsg * 3)]


# numpy view of cwslg_ft4_osd (72 bytes): three OSD_MSG_DTYPE records -- rec["set"]["crc_ok"][q, s] is set s of record q
FT4_OSD_DTYPE = np.dtype([("set", OSD_MSG_DTYPE, 3)])


def ft4_best_word(msg, osd):
    """The word a consumer takes from FT4 decode records (FT4_MSG_DTYPE) and the OSD records of the same entries (FT4_OSD_DTYPE): the smallest s
    with BP crc_ok (ft4_best_set); if there is none, the smallest s with OSD crc_ok, flagged by_osd (the bits are osd["set"][.., s]["bits"]
    then); -1 if neither stage has a word.  One record -> (int, bool), arrays of records -> (int array, bool array)."""
    bp = np.asarray(msg["set"]["crc_ok"]) != 0
    ok = np.asarray(osd["set"]["crc_ok"]) != 0
    has_bp = bp.any(axis=-1)
    by_osd = ~has_bp & ok.any(axis=-1)
    best = np.where(has_bp, bp.argmax(axis=-1), np.where(by_osd, ok.argmax(axis=-1), -1))
    return (int(best), bool(by_osd)) if best.ndim == 0 else (best.astype(np.int64), by_osd)


# numpy view of cwslg_decode (40 bytes): one de-duplicated decoded word of a channel, as cwslg_fetch_decodes hands them out
DECODE_DTYPE = np.dtype([("ch_id", np.int32), ("entry", np.int16), ("by_osd", np.uint8), ("set", np.uint8), ("bits", np.uint8, 12), ("freq_hz", np.float32),
                         ("dt_s", np.float32), ("sync", np.float32), ("dmin", np.float32), ("nharderr", np.int16), ("ndup", np.uint16)])
assert DECODE_DTYPE.itemsize == 40


# numpy views of cwslg_ap_pattern (24 bytes: mask and value over codeword bits 0..90, packed as a decode record's bits) and of cwslg_ap_msg
# (24 bytes: a decode record whose pad_ is the index of the pattern that succeeded, 0xff: none, and OSD's distance of the word found)
AP_PATTERN_DTYPE = np.dtype([("mask", np.uint8, 12), ("value", np.uint8, 12)])
AP_MSG_DTYPE = np.dtype([("msg", FT8_MSG_DTYPE), ("dmin", np.float32)])
assert AP_PATTERN_DTYPE.itemsize == 24 and AP_MSG_DTYPE.itemsize == 24


def merge_ap_decodes(decodes, ap):
    """What cwslg_fetch_ft8_ap (and cwslg_fetch_ft4_ap) leaves to the host: the records of fetch_decodes followed by those records of fetch_ft8_ap /
    fetch_ft4_ap (both DECODE_DTYPE, of one epoch and group) whose bits[12] no BP / OSD record of the same ch_id carries -- BP / OSD win -- in ascending (ch_id, entry), BP / OSD first
    where both name one entry's channel position."""
    decodes, ap = np.asarray(decodes, DECODE_DTYPE), np.asarray(ap, DECODE_DTYPE)
    have = {(int(d["ch_id"]), d["bits"].tobytes()) for d in decodes}
    keep = np.array([(int(a["ch_id"]), a["bits"].tobytes()) not in have for a in ap], bool)
    out = np.concatenate([decodes, ap[keep]])
    order = sorted(range(len(out)), key=lambda i: (int(out["ch_id"][i]), int(out["entry"][i]), int(out["by_osd"][i])))
    return out[order]


def ap_set_split(set_byte):
    """The `set` byte of an FT4 a-priori record (fetch_ft4_ap: by_osd = 2) -> (metric set, pattern index): set & 3, set >> 2.  Scalars or arrays."""
    v = np.asarray(set_byte).astype(np.int64)
    s, p = v & 3, v >> 2
    return (int(s), int(p)) if v.ndim == 0 else (s, p)


class DecodeReport(C.Structure):
    """cwslg_decode_report (16 bytes): the signal report of one cwslg_decode."""
    _fields_ = [("snr_db", C.c_float), ("xsig", C.c_float), ("xnoise", C.c_float), ("nsync", C.c_int16), ("nsymerr", C.c_int16)]


# numpy view of cwslg_decode_report, as cwslg_fetch_decode_reports hands them out: record p belongs to decode p
DECODE_REPORT_DTYPE = np.dtype([("snr_db", np.float32), ("xsig", np.float32), ("xnoise", np.float32), ("nsync", np.int16), ("nsymerr", np.int16)])
assert DECODE_REPORT_DTYPE.itemsize == 16 == C.sizeof(DecodeReport)
# numpy views of cwslg_subtract_report (record p belongs to decode p) and of cwslg_ft8_sub_item, the input of cwslg_ft8_subtract_flat
SUBTRACT_REPORT_DTYPE = np.dtype([("f_hz", np.float32), ("dt_s", np.float32), ("p_removed", np.float32), ("p_before", np.float32), ("p_after", np.float32),
                                  ("n_inside", np.int32), ("df_steps", np.int16), ("dt_steps", np.int16)])
FT8_SUB_ITEM_DTYPE = np.dtype([("frame", np.int32), ("bits", np.uint8, 12), ("freq_hz", np.float32), ("dt_s", np.float32)])
assert SUBTRACT_REPORT_DTYPE.itemsize == 28 and FT8_SUB_ITEM_DTYPE.itemsize == 24
# cwslg_ft4_sub_item, the input of cwslg_ft4_subtract_flat: the FT8 item's layout (freq_hz: a record's f1_hz); a frame is the decoder's 72576 samples
FT4_SUB_ITEM_DTYPE = np.dtype(FT8_SUB_ITEM_DTYPE.descr)
FT4_FRAME_SAMPLES = 72576
FT8_FRAME_SAMPLES = 180000


class Ft4Soft(C.Structure):
    _fields_ = [("llr", (C.c_float * 174) * 3), ("sigma", C.c_float * 3), ("nsync", C.c_int32), ("nqual", C.c_int32), ("pad_", C.c_int32)]


class WsprCandidate(C.Structure):
    _fields_ = [("freq_hz", C.c_float), ("snr_db", C.c_float), ("drift", C.c_float), ("sync", C.c_float), ("shift", C.c_int32)]


class Fst4wCandidate(C.Structure):
    _fields_ = [("freq_hz", C.c_float), ("snr", C.c_float), ("bin", C.c_int32), ("pad_", C.c_int32)]


class SlotResult(C.Structure):
    _fields_ = [("start_epoch", C.c_uint64), ("n_valid", C.c_uint64), ("factor", C.c_float), ("list_kind", C.c_int32),
                ("n_list", C.c_int32), ("n_ft4_sync", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("demod_launches", C.c_uint64), ("demod_samples", C.c_uint64),
                ("finalize_launches", C.c_uint64), ("sync_launches", C.c_uint64), ("frames_emitted", C.c_uint64),
                ("frames_discarded", C.c_uint64), ("blocks_dropped", C.c_uint64),
                ("h2d_bytes", C.c_uint64), ("demod_ms", C.c_double), ("finalize_ms", C.c_double),
                ("sync_ms", C.c_double), ("phasor_regrows", C.c_uint64), ("rendezvous_calls", C.c_uint64),
                ("rendezvous_frames", C.c_uint64), ("rccl_world", C.c_uint64), ("rendezvous_flags_and", C.c_uint64),
                ("demod_clock_mhz", C.c_double), ("demod_clock_launches", C.c_uint64), ("push_calls", C.c_uint64),
                ("push_batches", C.c_uint64), ("push_host_ms", C.c_double), ("sync_spectra_ms", C.c_double), ("sync_search_ms", C.c_double),
                ("demod_blocks_read", C.c_uint64), ("process_deferred", C.c_uint64)]


# int (*)(void *user, int group, uint64_t epoch_s, uint64_t frames_local, uint64_t *frames_total)
RENDEZVOUS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64))

_lib = None

# every symbol include/cwsl_gpu.h declares (tests check the library exports exactly these)
ABI_SYMBOLS = [
    "cwslg_abi_version", "cwslg_create", "cwslg_destroy", "cwslg_strerror", "cwslg_last_error",
    "cwslg_set_scale_factors", "cwslg_set_exact", "cwslg_receiver_open", "cwslg_receiver_close", "cwslg_push_iq", "cwslg_push_iq_many",
    "cwslg_push_iq_device", "cwslg_push_synth", "cwslg_ring_commit", "cwslg_ring_commit_all", "cwslg_ring_info", "cwslg_parse_decoder_line", "cwslg_channel_open_line", "cwslg_channel_open", "cwslg_channel_close", "cwslg_channel_tune", "cwslg_channel_tune_ex",
    "cwslg_channel_info", "cwslg_process", "cwslg_set_process_threshold", "cwslg_flush", "cwslg_exact_stream_length", "cwslg_slot_boundary", "cwslg_slot_boundary_begin", "cwslg_slot_boundary_end", "cwslg_slot_boundary_channel",
    "cwslg_set_boundary_rendezvous", "cwslg_set_rendezvous_flag", "cwslg_rccl_unique_id", "cwslg_rccl_init",
    "cwslg_enable_long_sync", "cwslg_fetch_wspr_candidates", "cwslg_fetch_fst4w_candidates", "cwslg_long_sync_debug_fetch",
    "cwslg_synchronize", "cwslg_fetch_frame", "cwslg_fetch_slot", "cwslg_write_wav", "cwslg_fetch_audio_f32", "cwslg_frame_device_ptrs",
    "cwslg_enable_sync", "cwslg_set_candidate_order", "cwslg_fetch_candidates", "cwslg_set_ft4_syncmin", "cwslg_enable_ft4_coherent", "cwslg_fetch_ft4_sync",
    "cwslg_enable_ft8_softbits", "cwslg_fetch_ft8_softbits", "cwslg_enable_ft4_softbits", "cwslg_fetch_ft4_softbits", "cwslg_sync_debug_fetch", "cwslg_get_stats", "cwslg_reset_stats",
    "cwslg_set_ldpc_code", "cwslg_enable_ft8_decode", "cwslg_fetch_ft8_decode", "cwslg_ldpc_decode",
    "cwslg_enable_ft8_osd", "cwslg_fetch_ft8_osd", "cwslg_osd_decode", "cwslg_enable_ft4_decode", "cwslg_fetch_ft4_decode",
    "cwslg_enable_ft4_osd", "cwslg_fetch_ft4_osd", "cwslg_fetch_decodes",
    "cwslg_fetch_decode_reports", "cwslg_ft8_tones", "cwslg_fetch_ft4_decode_reports", "cwslg_ft4_tones",
    "cwslg_set_ft8_ap", "cwslg_fetch_ft8_ap", "cwslg_ap_decode", "cwslg_set_ft4_ap", "cwslg_fetch_ft4_ap",
    "cwslg_subtract_ft8", "cwslg_fetch_ft8_residual", "cwslg_ft8_residual_device_ptr", "cwslg_ft8_subtract_flat",
    "cwslg_subtract_ft4", "cwslg_fetch_ft4_residual", "cwslg_ft4_residual_device_ptr", "cwslg_ft4_subtract_flat",
    "cwslg_set_timing", "cwslg_demod_kernel_name", "cwslg_stream", "cwslg_channel_constants", "cwslg_phasor_checkpoint_stride", "cwslg_channel_phasor_checkpoints",
    "cwslg_slot_clock_next", "cwslg_pool_sizing", "cwslg_find_band", "cwslg_parse_decode_line",
    "cwslg_decoder_block_bytes", "cwslg_decoder_block_field", "cwslg_fill_decoder_block", "cwslg_decoder_route", "cwslg_decoder_command",
]


def rccl_unique_id():
    """128-byte ncclUniqueId made by this process (rank 0 hands it to the other ranks)."""
    L = load_library()
    buf = C.create_string_buffer(128)
    rc = L.cwslg_rccl_unique_id(buf)
    if rc < 0:
        raise CwslGpuError(rc, L.cwslg_strerror(rc).decode())
    return buf.raw


def load_library(build_if_missing=True):
    """dlopen libcwslgpu.so.  Raises (never falls back) if it is absent and cannot be built."""
    global _lib
    if _lib is not None:
        return _lib
    if not build_if_missing and not os.path.isfile(_LIB_PATH):
        raise CwslGpuError(-7, f"{_LIB_PATH} not built")
    if build_if_missing and os.environ.get("CWSLG_LIB", "lab") == "lab":
        _build.build()          # returns at once when the library is newer than every source; serialised by a file lock
    try:
        # If torch is (or will be) in the process, let it load ITS libamdhip64 first: both copies carry
        # SONAME libamdhip64.so.7 and two HIP runtimes in one process do not share device pointers.
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(_LIB_PATH, mode=C.RTLD_GLOBAL)
    vp, i32, u32, u64, f32 = C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_float
    L.cwslg_abi_version.restype = i32
    L.cwslg_create.argtypes = [C.POINTER(vp), i32]
    L.cwslg_destroy.argtypes = [vp]; L.cwslg_destroy.restype = None
    L.cwslg_strerror.argtypes = [i32]; L.cwslg_strerror.restype = C.c_char_p
    L.cwslg_last_error.argtypes = [vp]; L.cwslg_last_error.restype = C.c_char_p
    L.cwslg_set_scale_factors.argtypes = [vp, f32, f32]
    L.cwslg_set_exact.argtypes = [vp, i32]
    L.cwslg_demod_kernel_name.argtypes = [vp]; L.cwslg_demod_kernel_name.restype = C.c_char_p
    L.cwslg_set_boundary_rendezvous.argtypes = [vp, RENDEZVOUS_FN, vp]
    L.cwslg_set_rendezvous_flag.argtypes = [vp, u64]
    L.cwslg_rccl_unique_id.argtypes = [vp]
    L.cwslg_rccl_init.argtypes = [vp, vp, i32, i32]
    L.cwslg_enable_long_sync.argtypes = [vp, i32, i32, i32, f32]
    L.cwslg_fetch_wspr_candidates.argtypes = [vp, i32, vp, i32, C.POINTER(i32), C.POINTER(u64)]
    L.cwslg_fetch_fst4w_candidates.argtypes = [vp, i32, vp, i32, C.POINTER(i32), C.POINTER(u64)]
    L.cwslg_fetch_slot.argtypes = [vp, i32, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(Ft4Sync), i32, C.POINTER(SlotResult)]
    L.cwslg_long_sync_debug_fetch.argtypes = [vp, i32, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.cwslg_receiver_open.argtypes = [vp, u32, u32, C.c_int32, u32, C.POINTER(i32)]
    L.cwslg_receiver_close.argtypes = [vp, i32]
    L.cwslg_push_iq.argtypes = [vp, i32, vp, u32]
    L.cwslg_push_iq_many.argtypes = [vp, i32, C.POINTER(i32), C.POINTER(vp), u32]
    L.cwslg_push_iq_device.argtypes = [vp, i32, vp, u32]
    L.cwslg_push_synth.argtypes = [vp, i32, u64, u32, u32, vp, i32, f32]
    L.cwslg_ring_commit.argtypes = [vp, i32, u32, u32]
    L.cwslg_ring_commit_all.argtypes = [vp, u32, u32]
    L.cwslg_ring_info.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u32), C.POINTER(u64)]
    L.cwslg_parse_decoder_line.argtypes = [C.c_char_p, C.c_double, C.POINTER(DecoderSpec)]
    L.cwslg_channel_open_line.argtypes = [vp, i32, C.c_char_p, C.c_double, C.POINTER(i32)]
    L.cwslg_channel_open.argtypes = [vp, i32, C.c_int32, i32, C.c_char_p, C.POINTER(i32)]
    L.cwslg_channel_close.argtypes = [vp, i32]
    L.cwslg_channel_tune.argtypes = [vp, i32, C.c_int32, i32]
    L.cwslg_channel_tune_ex.argtypes = [vp, i32, C.c_int32, i32, i32]
    L.cwslg_channel_info.argtypes = [vp, i32, C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(u32), C.POINTER(C.c_size_t)]
    L.cwslg_process.argtypes = [vp]
    L.cwslg_set_process_threshold.argtypes = [vp, i32]
    L.cwslg_flush.argtypes = [vp]
    L.cwslg_exact_stream_length.argtypes = [u64, u32, u32, i32]; L.cwslg_exact_stream_length.restype = u32
    L.cwslg_slot_boundary.argtypes = [vp, i32, u64]
    L.cwslg_slot_boundary_begin.argtypes = [vp, i32, u64]
    L.cwslg_slot_boundary_end.argtypes = [vp]
    L.cwslg_slot_boundary_channel.argtypes = [vp, i32, u64]
    L.cwslg_synchronize.argtypes = [vp]
    L.cwslg_fetch_frame.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(u64), C.POINTER(C.c_size_t), C.POINTER(f32)]
    L.cwslg_write_wav.argtypes = [vp, i32, C.c_char_p]
    L.cwslg_fetch_audio_f32.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.cwslg_frame_device_ptrs.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp)]
    L.cwslg_enable_sync.argtypes = [vp, i32, f32, i32, i32, i32]
    L.cwslg_fetch_candidates.argtypes = [vp, i32, C.POINTER(Candidate), i32, C.POINTER(i32), C.POINTER(u64)]
    L.cwslg_set_candidate_order.argtypes = [vp, i32]
    L.cwslg_set_ft4_syncmin.argtypes = [vp, f32]
    L.cwslg_enable_ft4_coherent.argtypes = [vp, i32]
    L.cwslg_fetch_ft4_sync.argtypes = [vp, i32, C.POINTER(Ft4Sync), i32, C.POINTER(i32), C.POINTER(u64)]
    L.cwslg_enable_ft8_softbits.argtypes = [vp, i32]
    L.cwslg_fetch_ft8_softbits.argtypes = [vp, i32, C.POINTER(Ft8Soft), i32, C.POINTER(i32), C.POINTER(u64)]
    L.cwslg_set_ldpc_code.argtypes = [vp, vp]
    L.cwslg_enable_ft8_decode.argtypes = [vp, i32, i32, i32]
    L.cwslg_fetch_ft8_decode.argtypes = [vp, i32, C.POINTER(Ft8Msg), i32, C.POINTER(i32), C.POINTER(u64)]
    L.cwslg_ldpc_decode.argtypes = [vp, vp, i32, i32, vp]
    L.cwslg_enable_ft8_osd.argtypes = [vp, i32, i32, i32]
    L.cwslg_fetch_ft8_osd.argtypes = [vp, i32, C.POINTER(OsdMsg), i32, C.POINTER(i32), C.POINTER(u64)]
    L.cwslg_osd_decode.argtypes = [vp, vp, i32, i32, vp]
    L.cwslg_enable_ft4_softbits.argtypes = [vp, i32]
    L.cwslg_fetch_ft4_softbits.argtypes = [vp, i32, C.POINTER(Ft4Soft), i32, C.POINTER(i32), C.POINTER(u64)]
    L.cwslg_enable_ft4_decode.argtypes = [vp, i32, i32, i32, i32]
    L.cwslg_fetch_ft4_decode.argtypes = [vp, i32, C.POINTER(Ft4Msg), i32, C.POINTER(i32), C.POINTER(u64)]
    L.cwslg_enable_ft4_osd.argtypes = [vp, i32, i32, i32, i32]
    L.cwslg_fetch_ft4_osd.argtypes = [vp, i32, C.POINTER(Ft4Osd), i32, C.POINTER(i32), C.POINTER(u64)]
    L.cwslg_fetch_decodes.argtypes = [vp, i32, C.POINTER(u64), vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.cwslg_fetch_decode_reports.argtypes = [vp, i32, C.POINTER(u64), vp, vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.cwslg_ft8_tones.argtypes = [vp, vp, vp]
    L.cwslg_subtract_ft8.argtypes = [vp, C.POINTER(u64), vp, vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.cwslg_fetch_ft8_residual.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(u64)]
    L.cwslg_ft8_residual_device_ptr.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u64)]
    L.cwslg_ft8_subtract_flat.argtypes = [vp, vp, i32, vp, i32, vp, vp]
    L.cwslg_subtract_ft4.argtypes = [vp, C.POINTER(u64), vp, vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.cwslg_fetch_ft4_residual.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(u64)]
    L.cwslg_ft4_residual_device_ptr.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(u64)]
    L.cwslg_ft4_subtract_flat.argtypes = [vp, vp, i32, vp, i32, vp, vp]
    L.cwslg_fetch_ft4_decode_reports.argtypes = [vp, C.POINTER(u64), vp, vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.cwslg_ft4_tones.argtypes = [vp, vp, vp]
    L.cwslg_set_ft8_ap.argtypes = [vp, vp, i32, i32, i32]
    L.cwslg_fetch_ft8_ap.argtypes = [vp, C.POINTER(u64), vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.cwslg_ap_decode.argtypes = [vp, vp, i32, vp]
    L.cwslg_set_ft4_ap.argtypes = [vp, vp, i32, i32, i32, i32]
    L.cwslg_fetch_ft4_ap.argtypes = [vp, C.POINTER(u64), vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    L.cwslg_sync_debug_fetch.argtypes = [vp, i32, i32, vp, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(i32)]
    L.cwslg_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.cwslg_reset_stats.argtypes = [vp]
    L.cwslg_set_timing.argtypes = [vp, i32]
    L.cwslg_stream.argtypes = [vp]; L.cwslg_stream.restype = vp
    L.cwslg_channel_constants.argtypes = [vp, i32, vp, vp, vp]
    L.cwslg_channel_phasor_checkpoints.argtypes = [vp, i32, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.cwslg_decoder_block_bytes.argtypes = [i32]; L.cwslg_decoder_block_bytes.restype = C.c_size_t
    L.cwslg_decoder_block_field.argtypes = [i32, C.c_char_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.cwslg_fill_decoder_block.argtypes = [vp, i32, vp, C.c_size_t, i32, i32, i32, C.POINTER(u64)]
    L.cwslg_decoder_route.argtypes = [C.c_char_p, i32]
    L.cwslg_decoder_command.argtypes = [C.c_char_p, i32, i32, i32, i32, i32, f32, C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    L.cwslg_parse_decode_line.argtypes = [C.c_char_p, C.c_char_p, C.c_int64, C.POINTER(Spot)]
    L.cwslg_slot_clock_next.argtypes = [i32, u64]; L.cwslg_slot_clock_next.restype = u64
    L.cwslg_pool_sizing.argtypes = [C.POINTER(i32), f32, i32, C.POINTER(i32), C.POINTER(i32)]
    L.cwslg_find_band.argtypes = [C.POINTER(C.c_int64), C.POINTER(u32), i32, C.c_int64]
    _lib = L
    return L


def parse_decode_line(mode, line, base_freq_hz):
    """One jt9 stdout line -> dict(status 'ok'|'unhandled'|'skip', snr_db, dt_s, freq_hz, call, locator, message)
    (OutputHandler.cpp:505-621, 924-1128)."""
    sp = Spot()
    rc = load_library().cwslg_parse_decode_line(mode.encode(), line.encode(), int(base_freq_hz), C.byref(sp))
    if rc < 0:
        raise CwslGpuError(rc, f"parse_decode_line({mode})")
    return dict(status=("ok", "unhandled", "skip")[rc], snr_db=sp.snr_db, dt_s=sp.dt_s, freq_hz=sp.freq_hz,
                call=sp.call.decode(), locator=sp.locator.decode() if sp.has_locator else None, message=sp.message.decode(), drift=sp.drift, dbm=sp.dbm)


def slot_clock_next(group, after_ms):
    """UTC ms of the group's (or mode's) next slot boundary strictly after after_ms (CWSL_DIGI.cpp:174-451)."""
    g = (GROUPS[group] if group in GROUPS else _MODE_GROUP[group]) if isinstance(group, str) else int(group)
    return int(load_library().cwslg_slot_clock_next(g, int(after_ms)))


POOL_ORDER = ("FT4", "FT8", "Q65-30", "JS8", "WSPR", "JT65", "FST4W", "FST4")


def pool_sizing(counts, decoderburden=1.0, n_decoders=None):
    """(numjt9instances, maxwsprdinstances) from decoder counts in POOL_ORDER (CWSL_DIGI.cpp:857-887)."""
    arr = (C.c_int * 8)(*[int(x) for x in counts])
    nj, nw = C.c_int(), C.c_int()
    rc = load_library().cwslg_pool_sizing(arr, float(decoderburden), int(sum(counts) if n_decoders is None else n_decoders),
                                          C.byref(nj), C.byref(nw))
    if rc != 0:
        raise CwslGpuError(rc, "pool_sizing")
    return nj.value, nw.value


def exact_stream_length(total_blocks, max_blocks, cu_count=256, latency=True):
    """cwslg_exact_stream_length: outputs per stream of the bit-identical kernel for a launch of that size (pure; no GPU needed)."""
    return int(load_library().cwslg_exact_stream_length(int(total_blocks), int(max_blocks), int(cu_count), 1 if latency else 0))


def find_band(bands, f_hz):
    """bands = [(lo_hz, fs_hz), ...]; index of the first band covering f_hz or -1 (CWSL_Utils.hpp:28-55)."""
    lo = (C.c_int64 * len(bands))(*[int(b[0]) for b in bands])
    fs = (C.c_uint32 * len(bands))(*[int(b[1]) for b in bands])
    return int(load_library().cwslg_find_band(lo, fs, len(bands), int(f_hz)))


def decoder_block_bytes(js8=False):
    """sizeof(dec_data_t) / sizeof(dec_data_js8_t) (DecoderPool.hpp:58-108 / :110-171)."""
    return load_library().cwslg_decoder_block_bytes(int(js8))


def decoder_block_field(name, js8=False):
    """(offset, bytes) of a member of the decoder block: ipc/ss/savg/sred/d2/params or a params field name."""
    off, n = C.c_size_t(), C.c_size_t()
    rc = load_library().cwslg_decoder_block_field(int(js8), name.encode(), C.byref(off), C.byref(n))
    if rc != 0:
        raise CwslGpuError(rc, f"no member {name!r} in the decoder block")
    return off.value, n.value


def decoder_route(mode, transfer_shmem=True):
    """'shmem' or 'wavefile' -- DecoderPool.hpp:379-395."""
    rc = load_library().cwslg_decoder_route(mode.encode(), int(transfer_shmem))
    if rc < 0:
        raise CwslGpuError(rc, f"Unhandled mode: {mode}")
    return "shmem" if rc == 1 else "wavefile"


def decoder_command(mode, target, shmem_route, numjt9threads=3, decodedepth=3, highest_decode_hz=3000, wspr_cycles=3000,
                    trperiod=0.0):
    """(program, argument string) exactly as DecoderPool.hpp:634-659 / :1007-1046 concatenate them."""
    app, opts = C.create_string_buffer(64), C.create_string_buffer(1024)
    rc = load_library().cwslg_decoder_command(mode.encode(), int(shmem_route), numjt9threads, decodedepth, highest_decode_hz,
                                              wspr_cycles, float(trperiod), str(target).encode(), app, 64, opts, 1024)
    if rc != 0:
        raise CwslGpuError(rc, f"Mode {mode} not handled")
    return app.value.decode(), opts.value.decode()


class Context:
    """One GPU's worth of receivers and channels (one process per GPU)."""

    def __init__(self, device=-1):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.cwslg_create(C.byref(h), device)
        if rc != 0:
            raise CwslGpuError(rc, self.L.cwslg_strerror(rc).decode())
        self.h = h
        self._modes = {}

    def close(self):
        if getattr(self, "h", None):
            self.L.cwslg_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise CwslGpuError(rc, self.L.cwslg_last_error(self.h).decode() or self.L.cwslg_strerror(rc).decode())
        return rc

    # ---- Receiver.hpp ----
    def receiver_open(self, fs=192000, iq_len=2048, lo_hz=0, ring_blocks=0):
        rid = C.c_int(-1)
        self._chk(self.L.cwslg_receiver_open(self.h, fs, iq_len, lo_hz, ring_blocks, C.byref(rid)))
        return rid.value

    def receiver_close(self, rx):
        self._chk(self.L.cwslg_receiver_close(self.h, rx))

    def push_iq(self, rx, iq):
        """iq: complex64[n] host array (one or more Receiver blocks)."""
        iq = np.ascontiguousarray(iq, dtype=np.complex64)
        self._chk(self.L.cwslg_push_iq(self.h, rx, iq.ctypes.data, iq.shape[0]))

    def push_iq_many(self, rxs, blocks):
        """One block per receiver in ONE call (cwslg_push_iq_many): rxs = receiver ids, blocks = complex64 arrays of one common length
        (or one 2-D array, row k for rxs[k])."""
        arrs = [np.ascontiguousarray(b, dtype=np.complex64) for b in blocks]
        n = arrs[0].shape[0]
        assert len(arrs) == len(rxs) and all(a.shape == (n,) for a in arrs)
        ids = (C.c_int * len(rxs))(*[int(r) for r in rxs])
        ptrs = (C.c_void_p * len(rxs))(*[a.ctypes.data for a in arrs])
        self._chk(self.L.cwslg_push_iq_many(self.h, len(rxs), ids, ptrs, n))

    def push_iq_device(self, rx, dptr, n_complex):
        self._chk(self.L.cwslg_push_iq_device(self.h, rx, C.c_void_p(dptr), n_complex))

    def push_synth(self, rx, seed, n_complex, block_len=0, tones_hz=(), amp=2.0e4):
        t = np.ascontiguousarray(tones_hz, dtype=np.float64)
        self._chk(self.L.cwslg_push_synth(self.h, rx, seed, n_complex, block_len,
                                          t.ctypes.data if len(t) else None, len(t), amp))

    def ring_commit(self, rx, n_complex, block_len=0):
        self._chk(self.L.cwslg_ring_commit(self.h, rx, n_complex, block_len))

    def ring_commit_all(self, n_complex, block_len=0):
        self._chk(self.L.cwslg_ring_commit_all(self.h, n_complex, block_len))

    def ring_info(self, rx):
        p, cap, tot = C.c_void_p(), C.c_uint32(), C.c_uint64()
        self._chk(self.L.cwslg_ring_info(self.h, rx, C.byref(p), C.byref(cap), C.byref(tot)))
        return p.value, cap.value, tot.value

    # ---- Instance.cpp / SSBD.hpp ----
    def channel_open(self, rx, demod_hz, mode="FT8", usb=True):
        cid = C.c_int(-1)
        self._chk(self.L.cwslg_channel_open(self.h, rx, int(demod_hz), 1 if usb else 0, mode.encode(), C.byref(cid)))
        self._modes[cid.value] = mode
        return cid.value

    def channel_open_line(self, rx, line, freqcal_global=1.0):
        """Open a channel from an unchanged config.ini `decoder=` value."""
        cid = C.c_int(-1)
        self._chk(self.L.cwslg_channel_open_line(self.h, rx, line.encode(), float(freqcal_global), C.byref(cid)))
        self._modes[cid.value] = parse_decoder_line(line, freqcal_global)["mode"]
        return cid.value

    def channel_close(self, ch):
        self._chk(self.L.cwslg_channel_close(self.h, ch))
        self._modes.pop(ch, None)

    def channel_tune(self, ch, demod_hz, usb=True, reset=True):
        """SSBD::Tune(F, isUSB, reset): retune in place; reset=True restarts history and phasor, reset=False keeps them
        (SSBD.hpp:96-123)."""
        self._chk(self.L.cwslg_channel_tune_ex(self.h, ch, int(demod_hz), 1 if usb else 0, 1 if reset else 0))

    def channel_info(self, ch):
        a, b, c_, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        fl = C.c_size_t()
        self._chk(self.L.cwslg_channel_info(self.h, ch, C.byref(a), C.byref(b), C.byref(c_), C.byref(d), C.byref(fl)))
        return dict(in_size=a.value, out_size=b.value, out_rate=c_.value, delay=d.value, frame_len=fl.value)

    def process(self):
        self._chk(self.L.cwslg_process(self.h))

    def flush(self):
        """cwslg_flush: demodulate everything pending now, whatever the process threshold."""
        self._chk(self.L.cwslg_flush(self.h))

    def set_process_threshold(self, min_outputs=-1):
        """cwslg_set_process_threshold: 0 every process() launches; > 0 only once a channel has that many outputs pending; < 0 the library's own."""
        self._chk(self.L.cwslg_set_process_threshold(self.h, int(min_outputs)))

    def slot_boundary(self, group, epoch_s):
        if isinstance(group, str):                       # a group name ("S120") or a mode name ("WSPR" -> its group)
            g = GROUPS[group] if group in GROUPS else _MODE_GROUP[group]
        else:
            g = int(group)
        self._chk(self.L.cwslg_slot_boundary(self.h, g, int(epoch_s)))

    def slot_boundary_begin(self, group, epoch_s):
        """First half of slot_boundary: queue the boundary's device work, return at once (see cwslg_slot_boundary_begin)."""
        g = (GROUPS[group] if group in GROUPS else _MODE_GROUP[group]) if isinstance(group, str) else int(group)
        self._chk(self.L.cwslg_slot_boundary_begin(self.h, g, int(epoch_s)))

    def slot_boundary_end(self):
        """Second half: wait for that boundary's kernels and run the rendezvous."""
        self._chk(self.L.cwslg_slot_boundary_end(self.h))

    def set_boundary_rendezvous(self, fn):
        """Install the multi-GPU slot-boundary rendezvous: fn(group, epoch_s, frames_local) -> frames over all
        processes (e.g. shard.slot_boundary_rendezvous over torch.distributed).  None removes it."""
        if fn is None:
            self._rdv_cb = None
            self._chk(self.L.cwslg_set_boundary_rendezvous(self.h, RENDEZVOUS_FN(), None))
            return

        def tramp(_user, group, epoch_s, frames_local, total_out):
            try:
                total_out[0] = int(fn(int(group), int(epoch_s), int(frames_local)))
                return 0
            except Exception:                              # an exception must not unwind through the C caller
                import traceback
                traceback.print_exc()
                return ERR_HIP
        self._rdv_cb = RENDEZVOUS_FN(tramp)                 # keep the trampoline alive as long as it is installed
        self._chk(self.L.cwslg_set_boundary_rendezvous(self.h, self._rdv_cb, None))

    def set_rendezvous_flag(self, flag):
        """The 64-bit word this process contributes to every later built-in rendezvous (stats()["rendezvous_flags_and"])."""
        self._chk(self.L.cwslg_set_rendezvous_flag(self.h, int(flag)))

    def rccl_init(self, unique_id, rank, world):
        """Built-in RCCL rendezvous (what a C++ host uses): unique_id = bytes from rccl_unique_id() of rank 0."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._chk(self.L.cwslg_rccl_init(self.h, buf, int(rank), int(world)))

    def slot_boundary_channel(self, ch, epoch_s):
        self._chk(self.L.cwslg_slot_boundary_channel(self.h, ch, int(epoch_s)))

    def synchronize(self):
        self._chk(self.L.cwslg_synchronize(self.h))

    def fetch_frame(self, ch):
        """-> None until a frame was finalised, else dict(i16, t_start, n_valid, factor)."""
        n = frame_len(self._modes[ch])
        out = np.empty(n, np.int16)
        t0, nv, fac = C.c_uint64(), C.c_size_t(), C.c_float()
        rc = self.L.cwslg_fetch_frame(self.h, ch, out.ctypes.data, n, C.byref(t0), C.byref(nv), C.byref(fac))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return dict(i16=out, t_start=t0.value, n_valid=nv.value, factor=np.float32(fac.value))

    def write_wav(self, ch, path):
        """The reference's 46-byte-header 12 kHz mono int16 .wav of the last finalised frame (WaveFile.hpp:87-135)."""
        self._chk(self.L.cwslg_write_wav(self.h, ch, str(path).encode()))

    def fill_decoder_block(self, ch, block=None, js8=False, decodedepth=3, highest_decode_hz=3000):
        """The jt9/js8 shared-memory block for the last finalised frame (DecoderPool.hpp:451-590).  `block` is a
        writable uint8 array of decoder_block_bytes(js8) (e.g. a mapped shared-memory segment) or None to allocate.
        Returns (block, t_start) or None before the first frame."""
        n = decoder_block_bytes(js8)
        if block is None:
            block = np.empty(n, np.uint8)
        t0 = C.c_uint64()
        rc = self.L.cwslg_fill_decoder_block(self.h, ch, block.ctypes.data, block.nbytes, int(js8), decodedepth,
                                             highest_decode_hz, C.byref(t0))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return block, t0.value

    def fetch_audio_f32(self, ch):
        n = frame_len(self._modes[ch])
        out = np.empty(n, np.float32)
        nv = C.c_size_t()
        rc = self.L.cwslg_fetch_audio_f32(self.h, ch, out.ctypes.data, n, C.byref(nv))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return out, nv.value

    def frame_device_ptrs(self, ch):
        a, b = C.c_void_p(), C.c_void_p()
        self._chk(self.L.cwslg_frame_device_ptrs(self.h, ch, C.byref(a), C.byref(b)))
        return a.value, b.value

    def enable_sync(self, enable=True, syncmin=1.5, max_cand=200, f_lo_hz=200, f_hi_hz=3000):
        self._chk(self.L.cwslg_enable_sync(self.h, 1 if enable else 0, syncmin, max_cand, f_lo_hz, f_hi_hz))

    def set_candidate_order(self, order="sync"):
        """'sync' (default): strongest first, cut at max_cand in that order; 'freq': ascending frequency, cut in THAT order."""
        self._chk(self.L.cwslg_set_candidate_order(self.h, {"sync": 0, "freq": 1}[order]))

    def _fetch_records(self, fn, ch, buf, max_items, none_without_frame=True):
        """One list / record fetch of the C ABI into buf: -> (n, start epoch), or None for CWSLG_ERR_NO_FRAME (raised like every other error
        with none_without_frame=False)."""
        n = C.c_int()
        t0 = C.c_uint64()
        rc = fn(self.h, ch, buf, int(max_items), C.byref(n), C.byref(t0))
        if rc == ERR_NO_FRAME and none_without_frame:
            return None
        self._chk(rc)
        return n.value, t0.value

    def fetch_candidates(self, ch, max_cand=600, with_epoch=False):
        """[(freq_bin, time_step, sync, freq_hz, dt_s)]; with_epoch: (list, start epoch of the frame the list was computed from)."""
        buf = (Candidate * max_cand)()
        n, t0 = self._fetch_records(self.L.cwslg_fetch_candidates, ch, buf, max_cand, none_without_frame=False)
        out = [(buf[k].freq_bin, buf[k].time_step, buf[k].sync, buf[k].freq_hz, buf[k].dt_s) for k in range(n)]
        return (out, t0) if with_epoch else out

    def fetch_slot(self, ch, max_list=1000, max_ft4=3000, want_frame=True):
        """cwslg_fetch_slot: frame + candidate list(s) of ONE epoch under one ticket.  -> None before the first frame, else a dict with
        i16 (or None), t_start, n_valid, factor, list_kind ('none' / 'FT8' / 'FT4' / 'WSPR' / 'FST4W'), list (tuples in the layout of the
        matching fetch_*_candidates call) and ft4_sync (dicts as fetch_ft4_sync)."""
        n = frame_len(self._modes[ch])
        out = np.empty(n, np.int16) if want_frame else None
        item = max(C.sizeof(Candidate), C.sizeof(WsprCandidate), C.sizeof(Fst4wCandidate))
        raw = (C.c_char * (item * max_list))()
        ft4 = (Ft4Sync * max_ft4)()
        res = SlotResult()
        rc = self.L.cwslg_fetch_slot(self.h, ch, out.ctypes.data if want_frame else None, n if want_frame else 0, raw, len(raw), ft4, max_ft4, C.byref(res))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        kind = ("none", "FT8", "FT4", "WSPR", "FST4W")[res.list_kind]
        lst = []
        if kind in ("FT8", "FT4"):
            b = C.cast(raw, C.POINTER(Candidate))
            lst = [(b[k].freq_bin, b[k].time_step, b[k].sync, b[k].freq_hz, b[k].dt_s) for k in range(res.n_list)]
        elif kind == "WSPR":
            b = C.cast(raw, C.POINTER(WsprCandidate))
            lst = [(b[k].freq_hz, b[k].snr_db, b[k].drift, b[k].sync, b[k].shift) for k in range(res.n_list)]
        elif kind == "FST4W":
            b = C.cast(raw, C.POINTER(Fst4wCandidate))
            lst = [(b[k].freq_hz, b[k].snr, b[k].bin) for k in range(res.n_list)]
        f4 = [dict(f0_hz=b.f0_hz, f1_hz=b.f1_hz, dt_s=b.dt_s, sync=b.sync, ibest=b.ibest, idf=b.idf, seg=b.seg, cand=b.cand) for b in ft4[:res.n_ft4_sync]]
        return dict(i16=out, t_start=res.start_epoch, n_valid=res.n_valid, factor=res.factor, list_kind=kind, list=lst, ft4_sync=f4)

    def enable_ft4_coherent(self, enable=True):
        self._chk(self.L.cwslg_enable_ft4_coherent(self.h, int(enable)))

    def fetch_ft4_sync(self, ch, max_rec=1800, with_epoch=False):
        """Refined FT4 candidates (ft4_downsample + sync4d search): list of dicts, candidate order then segment order; None unless the coherent
        stage ran on the list now on the device (with_epoch: (list, start epoch of the frame the records were computed from))."""
        buf = (Ft4Sync * max_rec)()
        r = self._fetch_records(self.L.cwslg_fetch_ft4_sync, ch, buf, max_rec)
        if r is None:
            return None
        n, t0 = r
        out = [dict(f0_hz=b.f0_hz, f1_hz=b.f1_hz, dt_s=b.dt_s, sync=b.sync, ibest=b.ibest, idf=b.idf, seg=b.seg, cand=b.cand)
               for b in buf[:n]]
        return (out, t0) if with_epoch else out

    def enable_ft8_softbits(self, enable=True):
        """Soft bits per FT8 sync candidate (cwslg_ft8_soft); needs enable_sync; applies from the next boundary on."""
        self._chk(self.L.cwslg_enable_ft8_softbits(self.h, int(enable)))

    def fetch_ft8_softbits(self, ch, max_cand=600, with_epoch=False):
        """-> None unless soft-bit records of the channel's current epoch exist, else (llr float32[n, 174], sigma float32[n], nsync int32[n]):
        row q belongs to entry q of fetch_candidates' list of the same epoch (with_epoch: the frame's start epoch as a fourth item)."""
        buf = np.zeros((max(int(max_cand), 1), 176), np.float32)          # one 704-byte record per row
        r = self._fetch_records(self.L.cwslg_fetch_ft8_softbits, ch, buf.ctypes.data_as(C.POINTER(Ft8Soft)), int(max_cand))
        if r is None:
            return None
        n, t0 = r
        rec = buf[:n]
        out = (np.ascontiguousarray(rec[:, :174]), rec[:, 174].copy(), rec[:, 175].copy().view(np.int32))
        return out + (t0,) if with_epoch else out

    def set_ldpc_code(self, nm):
        """Load the (174, 91) parity-check table: nm uint8[83, 7], 1-based codeword positions, a row of weight 6 ends in one 0 (the integrator's own
        copy of WSJT-X's Nm).  Raises ERR_ARG for a table that fails validation; the code loaded before stays."""
        nm = np.ascontiguousarray(nm, dtype=np.uint8)
        if nm.size != 83 * 7:
            raise CwslGpuError(-6, "the parity-check table is 83 x 7")
        self._chk(self.L.cwslg_set_ldpc_code(self.h, nm.ctypes.data))

    def enable_ft8_decode(self, enable=True, max_iter=30, min_nsync=7):
        """LDPC decode + CRC-14 per FT8 sync candidate (cwslg_ft8_msg); needs a loaded code, enable_sync and enable_ft8_softbits; applies from the
        next boundary on."""
        self._chk(self.L.cwslg_enable_ft8_decode(self.h, int(enable), int(max_iter), int(min_nsync)))

    def fetch_ft8_decode(self, ch, max_cand=600, with_epoch=False):
        """-> None unless decode records of the channel's current epoch exist, else a numpy record array (FT8_MSG_DTYPE: bits uint8[12], iters, nbad,
        nharderr, crc_ok) whose row q belongs to entry q of fetch_candidates' list of the same epoch (with_epoch: (records, frame start epoch))."""
        buf = np.zeros(max(int(max_cand), 1), FT8_MSG_DTYPE)
        r = self._fetch_records(self.L.cwslg_fetch_ft8_decode, ch, buf.ctypes.data_as(C.POINTER(Ft8Msg)), int(max_cand))
        if r is None:
            return None
        n, t0 = r
        rec = buf[:n].copy()
        return (rec, t0) if with_epoch else rec

    def ldpc_decode(self, llr, max_iter=30):
        """The decode kernel on caller-supplied metrics, llr float32[n, 174] (n >= 0), no nsync filter; synchronous.  -> record array [n]."""
        llr = np.ascontiguousarray(llr, dtype=np.float32).reshape(-1, 174)
        out = np.zeros(len(llr), FT8_MSG_DTYPE)
        self._chk(self.L.cwslg_ldpc_decode(self.h, llr.ctypes.data if len(llr) else None, len(llr), int(max_iter), out.ctypes.data if len(llr) else None))
        return out

    def enable_ft8_osd(self, enable=True, order=2, min_nsync=7):
        """Ordered-statistics decoding (order 0..2) of the FT8 candidates the decode attempted without crc_ok (cwslg_osd_msg); needs a loaded code of
        rank 83; runs at the boundaries at which enable_ft8_softbits and enable_ft8_decode are on too."""
        self._chk(self.L.cwslg_enable_ft8_osd(self.h, int(enable), int(order), int(min_nsync)))

    def fetch_ft8_osd(self, ch, max_cand=600, with_epoch=False):
        """-> None unless OSD records of the channel's current epoch exist, else a numpy record array (OSD_MSG_DTYPE: bits uint8[12], dmin, nharderr,
        nskip, crc_ok, how, flip uint8[2]) whose row q belongs to entry q of fetch_candidates' list of the same epoch (with_epoch: (records, frame
        start epoch))."""
        buf = np.zeros(max(int(max_cand), 1), OSD_MSG_DTYPE)
        r = self._fetch_records(self.L.cwslg_fetch_ft8_osd, ch, buf.ctypes.data_as(C.POINTER(OsdMsg)), int(max_cand))
        if r is None:
            return None
        n, t0 = r
        rec = buf[:n].copy()
        return (rec, t0) if with_epoch else rec

    def osd_decode(self, llr, order=2):
        """The OSD kernel on caller-supplied metrics, llr float32[n, 174] (n >= 0), no gates; synchronous.  -> record array [n]."""
        llr = np.ascontiguousarray(llr, dtype=np.float32).reshape(-1, 174)
        out = np.zeros(len(llr), OSD_MSG_DTYPE)
        self._chk(self.L.cwslg_osd_decode(self.h, llr.ctypes.data if len(llr) else None, len(llr), int(order), out.ctypes.data if len(llr) else None))
        return out

    def enable_ft4_softbits(self, enable=True):
        """Soft bits per refined FT4 sync record (cwslg_ft4_soft); needs enable_sync; applies from the next boundary on."""
        self._chk(self.L.cwslg_enable_ft4_softbits(self.h, int(enable)))

    def fetch_ft4_softbits(self, ch, max_rec=1800, with_epoch=False):
        """-> None unless soft-bit records of the channel's current epoch exist, else (llr float32[n, 3, 174], sigma float32[n, 3],
        nsync int32[n], nqual int32[n]): row q belongs to entry q of fetch_ft4_sync of the same epoch (with_epoch: the frame's start epoch
        as a fifth item)."""
        buf = np.zeros((max(int(max_rec), 1), 528), np.float32)           # one 2112-byte record per row
        r = self._fetch_records(self.L.cwslg_fetch_ft4_softbits, ch, buf.ctypes.data_as(C.POINTER(Ft4Soft)), int(max_rec))
        if r is None:
            return None
        n, t0 = r
        rec = buf[:n]
        out = (np.ascontiguousarray(rec[:, :522]).reshape(-1, 3, 174), np.ascontiguousarray(rec[:, 522:525]),
               rec[:, 525].copy().view(np.int32), rec[:, 526].copy().view(np.int32))
        return out + (t0,) if with_epoch else out

    def enable_ft4_decode(self, enable=True, max_iter=30, min_nsync=8, min_nqual=20):
        """LDPC decode + CRC-14 on the three metric sets of every FT4 soft-bit record (cwslg_ft4_msg); needs a loaded code, enable_sync and
        enable_ft4_softbits; applies from the next boundary on."""
        self._chk(self.L.cwslg_enable_ft4_decode(self.h, int(enable), int(max_iter), int(min_nsync), int(min_nqual)))

    def fetch_ft4_decode(self, ch, max_rec=1800, with_epoch=False):
        """-> None unless decode records of the channel's current epoch exist, else a numpy record array (FT4_MSG_DTYPE: rec["set"][q, s] is the
        FT8_MSG_DTYPE record of metric set s) whose row q belongs to entry q of fetch_ft4_sync of the same epoch (with_epoch: (records, frame
        start epoch)).  ft4_best_set picks the set upstream would take."""
        buf = np.zeros(max(int(max_rec), 1), FT4_MSG_DTYPE)
        r = self._fetch_records(self.L.cwslg_fetch_ft4_decode, ch, buf.ctypes.data_as(C.POINTER(Ft4Msg)), int(max_rec))
        if r is None:
            return None
        n, t0 = r
        rec = buf[:n].copy()
        return (rec, t0) if with_epoch else rec

    def enable_ft4_osd(self, enable=True, order=2, min_nsync=8, min_nqual=20):
        """Ordered-statistics decoding (order 0..2) of the metric sets of the FT4 records no set of which the decode brought to crc_ok
        (cwslg_ft4_osd); needs a loaded code of rank 83; runs at boundaries where the coherent stage, enable_ft4_softbits and enable_ft4_decode are on
        too."""
        self._chk(self.L.cwslg_enable_ft4_osd(self.h, int(enable), int(order), int(min_nsync), int(min_nqual)))

    def fetch_ft4_osd(self, ch, max_rec=1800, with_epoch=False):
        """-> None unless OSD records of the channel's current epoch exist, else a numpy record array (FT4_OSD_DTYPE: rec["set"][q, s] is the
        OSD_MSG_DTYPE record of metric set s) whose row q belongs to entry q of fetch_ft4_sync of the same epoch (with_epoch: (records, frame
        start epoch)).  ft4_best_word picks the word a consumer takes from the decode and OSD records together."""
        buf = np.zeros(max(int(max_rec), 1), FT4_OSD_DTYPE)
        r = self._fetch_records(self.L.cwslg_fetch_ft4_osd, ch, buf.ctypes.data_as(C.POINTER(Ft4Osd)), int(max_rec))
        if r is None:
            return None
        n, t0 = r
        rec = buf[:n].copy()
        return (rec, t0) if with_epoch else rec

    def fetch_decodes(self, group, start_epoch=0, max=4096):
        """cwslg_fetch_decodes: the decoded words of a whole FT8 / FT4 slot-clock group ("FT8" / "FT4" or a group number) in one fetch, chosen
        (BP before OSD) and de-duplicated per channel on the device.  start_epoch 0: the newest epoch any channel of the group has decode records
        of.  -> None if no channel takes part (CWSLG_ERR_NO_FRAME), else (records, start_epoch, n_total, n_channels): records a numpy array
        (DECODE_DTYPE) of the first min(n_total, max) decodes in ascending (ch_id, entry)."""
        g = (GROUPS[group] if group in GROUPS else _MODE_GROUP[group]) if isinstance(group, str) else int(group)
        buf = np.zeros(int(max) if int(max) > 1 else 1, DECODE_DTYPE)
        t0, n, n_total, n_ch = C.c_uint64(int(start_epoch)), C.c_int(), C.c_int(), C.c_int()
        rc = self.L.cwslg_fetch_decodes(self.h, g, C.byref(t0), buf.ctypes.data if int(max) > 0 else None, int(max), C.byref(n), C.byref(n_total), C.byref(n_ch))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return buf[:n.value].copy(), t0.value, n_total.value, n_ch.value

    def fetch_decode_reports(self, group="FT8", start_epoch=0, max=4096):
        """cwslg_fetch_decode_reports: fetch_decodes with a signal report per decode (FT8 group only; needs a systematic code loaded).  -> None if
        no channel takes part, else (records, reports, start_epoch, n_total, n_channels): reports a numpy array (DECODE_REPORT_DTYPE), reports[p]
        the SNR figure, xsig / xnoise and the nsync / nsymerr tone checks of records[p]."""
        g = (GROUPS[group] if group in GROUPS else _MODE_GROUP[group]) if isinstance(group, str) else int(group)
        m = int(max)
        dec, rep = np.zeros(m if m > 1 else 1, DECODE_DTYPE), np.zeros(m if m > 1 else 1, DECODE_REPORT_DTYPE)
        t0, n, n_total, n_ch = C.c_uint64(int(start_epoch)), C.c_int(), C.c_int(), C.c_int()
        rc = self.L.cwslg_fetch_decode_reports(self.h, g, C.byref(t0), dec.ctypes.data if m > 0 else None, rep.ctypes.data if m > 0 else None, m,
                                               C.byref(n), C.byref(n_total), C.byref(n_ch))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return dec[:n.value].copy(), rep[:n.value].copy(), t0.value, n_total.value, n_ch.value

    def subtract_ft8(self, start_epoch=0, max=4096):
        """cwslg_subtract_ft8: fetch_decodes("FT8") with a refined fit per decode, and a residual frame left on the device for every channel that
        took part (fetch_ft8_residual).  Needs a systematic code loaded.  -> None if no channel takes part, else (records, sub, start_epoch,
        n_total, n_channels): sub a numpy array (SUBTRACT_REPORT_DTYPE), sub[p] the refined f_hz / dt_s and the energy figures of records[p]."""
        m = int(max)
        dec, sub = np.zeros(m if m > 1 else 1, DECODE_DTYPE), np.zeros(m if m > 1 else 1, SUBTRACT_REPORT_DTYPE)
        t0, n, n_total, n_ch = C.c_uint64(int(start_epoch)), C.c_int(), C.c_int(), C.c_int()
        rc = self.L.cwslg_subtract_ft8(self.h, C.byref(t0), dec.ctypes.data if m > 0 else None, sub.ctypes.data if m > 0 else None, m,
                                       C.byref(n), C.byref(n_total), C.byref(n_ch))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return dec[:n.value].copy(), sub[:n.value].copy(), t0.value, n_total.value, n_ch.value

    def fetch_ft8_residual(self, ch):
        """cwslg_fetch_ft8_residual: the channel's residual frame of the last subtract_ft8 -> (float32[180000], start_epoch), or None once the
        channel's frame is of another epoch (or the channel did not take part)."""
        out = np.zeros(FT8_FRAME_SAMPLES, np.float32)
        nv, t0 = C.c_size_t(), C.c_uint64()
        rc = self.L.cwslg_fetch_ft8_residual(self.h, int(ch), out.ctypes.data, out.size, C.byref(nv), C.byref(t0))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return out, t0.value

    def ft8_residual_device_ptr(self, ch):
        """cwslg_ft8_residual_device_ptr -> (device address of the channel's residual, start_epoch), or None (as fetch_ft8_residual)."""
        p, t0 = C.c_void_p(), C.c_uint64()
        rc = self.L.cwslg_ft8_residual_device_ptr(self.h, int(ch), C.byref(p), C.byref(t0))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return p.value, t0.value

    def ft8_subtract_flat(self, audio, items, want_residual=True):
        """cwslg_ft8_subtract_flat: the subtractor's two kernels on caller-supplied frames.  audio: float32 [n_frames][180000]; items: an array of
        FT8_SUB_ITEM_DTYPE (or tuples (frame, bits[12], freq_hz, dt_s)) in ascending frame order.  -> (sub SUBTRACT_REPORT_DTYPE[n_items],
        residual float32 [n_frames][180000] or None)."""
        a = np.ascontiguousarray(audio, np.float32)
        if a.ndim == 1:
            a = a.reshape(1, -1)
        if a.ndim != 2 or a.shape[1] != FT8_FRAME_SAMPLES:
            raise ValueError("audio: [n_frames][180000]")
        it = np.ascontiguousarray(np.asarray(items, FT8_SUB_ITEM_DTYPE).reshape(-1))
        sub = np.zeros(max(it.size, 1), SUBTRACT_REPORT_DTYPE)
        res = np.zeros_like(a) if want_residual else None
        self._chk(self.L.cwslg_ft8_subtract_flat(self.h, a.ctypes.data, a.shape[0], it.ctypes.data if it.size else None, it.size,
                                                 sub.ctypes.data if it.size else None, res.ctypes.data if want_residual else None))
        return sub[:it.size].copy(), res

    def subtract_ft4(self, start_epoch=0, max=4096):
        """cwslg_subtract_ft4: fetch_decodes("FT4") with a refined fit per decode, and a residual frame left on the device for every FT4 channel
        that took part (fetch_ft4_residual).  Needs a systematic code loaded.  -> None if no channel takes part, else (records, sub, start_epoch,
        n_total, n_channels), as subtract_ft8."""
        m = int(max)
        dec, sub = np.zeros(m if m > 1 else 1, DECODE_DTYPE), np.zeros(m if m > 1 else 1, SUBTRACT_REPORT_DTYPE)
        t0, n, n_total, n_ch = C.c_uint64(int(start_epoch)), C.c_int(), C.c_int(), C.c_int()
        rc = self.L.cwslg_subtract_ft4(self.h, C.byref(t0), dec.ctypes.data if m > 0 else None, sub.ctypes.data if m > 0 else None, m,
                                       C.byref(n), C.byref(n_total), C.byref(n_ch))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return dec[:n.value].copy(), sub[:n.value].copy(), t0.value, n_total.value, n_ch.value

    def fetch_ft4_residual(self, ch):
        """cwslg_fetch_ft4_residual: the channel's residual frame of the last subtract_ft4 -> (float32[72576], start_epoch), or None once the
        channel's frame is of another epoch (or the channel did not take part, or is no FT4 channel)."""
        out = np.zeros(FT4_FRAME_SAMPLES, np.float32)
        nv, t0 = C.c_size_t(), C.c_uint64()
        rc = self.L.cwslg_fetch_ft4_residual(self.h, int(ch), out.ctypes.data, out.size, C.byref(nv), C.byref(t0))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return out, t0.value

    def ft4_residual_device_ptr(self, ch):
        """cwslg_ft4_residual_device_ptr -> (device address of the channel's residual, start_epoch), or None (as fetch_ft4_residual)."""
        p, t0 = C.c_void_p(), C.c_uint64()
        rc = self.L.cwslg_ft4_residual_device_ptr(self.h, int(ch), C.byref(p), C.byref(t0))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return p.value, t0.value

    def ft4_subtract_flat(self, audio, items, want_residual=True):
        """cwslg_ft4_subtract_flat: the FT4 subtractor's two kernels on caller-supplied frames.  audio: float32 [n_frames][72576]; items: an array
        of FT4_SUB_ITEM_DTYPE (or tuples (frame, bits[12], f1_hz, dt_s)) in ascending frame order.  -> (sub SUBTRACT_REPORT_DTYPE[n_items],
        residual float32 [n_frames][72576] or None)."""
        a = np.ascontiguousarray(audio, np.float32)
        if a.ndim == 1:
            a = a.reshape(1, -1)
        if a.ndim != 2 or a.shape[1] != FT4_FRAME_SAMPLES:
            raise ValueError("audio: [n_frames][72576]")
        it = np.ascontiguousarray(np.asarray(items, FT4_SUB_ITEM_DTYPE).reshape(-1))
        sub = np.zeros(max(it.size, 1), SUBTRACT_REPORT_DTYPE)
        res = np.zeros_like(a) if want_residual else None
        self._chk(self.L.cwslg_ft4_subtract_flat(self.h, a.ctypes.data, a.shape[0], it.ctypes.data if it.size else None, it.size,
                                                 sub.ctypes.data if it.size else None, res.ctypes.data if want_residual else None))
        return sub[:it.size].copy(), res

    def ft8_tones(self, bits):
        """cwslg_ft8_tones: the 79 channel tones of a 91-bit word (bits[12] as in a decode record) under the code in force -> uint8[79]."""
        b = np.ascontiguousarray(np.frombuffer(bytes(bits), np.uint8) if isinstance(bits, (bytes, bytearray)) else np.asarray(bits, np.uint8))
        if b.shape != (12,):
            raise ValueError("bits: 12 bytes")
        tones = np.zeros(79, np.uint8)
        self._chk(self.L.cwslg_ft8_tones(self.h, b.ctypes.data, tones.ctypes.data))
        return tones

    def fetch_ft4_decode_reports(self, start_epoch=0, max=4096):
        """cwslg_fetch_ft4_decode_reports: fetch_decodes("FT4") with a signal report per decode (needs a systematic code loaded).  -> None if no
        channel takes part, else (records, reports, start_epoch, n_total, n_channels): reports a numpy array (DECODE_REPORT_DTYPE), reports[p] the
        SNR figure (never below -21), xsig / xnoise and the nsync (0..16) / nsymerr (0..87) tone checks of records[p]."""
        m = int(max)
        dec, rep = np.zeros(m if m > 1 else 1, DECODE_DTYPE), np.zeros(m if m > 1 else 1, DECODE_REPORT_DTYPE)
        t0, n, n_total, n_ch = C.c_uint64(int(start_epoch)), C.c_int(), C.c_int(), C.c_int()
        rc = self.L.cwslg_fetch_ft4_decode_reports(self.h, C.byref(t0), dec.ctypes.data if m > 0 else None, rep.ctypes.data if m > 0 else None, m,
                                                   C.byref(n), C.byref(n_total), C.byref(n_ch))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return dec[:n.value].copy(), rep[:n.value].copy(), t0.value, n_total.value, n_ch.value

    @staticmethod
    def _ap_patterns(patterns):
        pat = np.zeros(len(patterns), AP_PATTERN_DTYPE)
        if isinstance(patterns, np.ndarray) and patterns.dtype == AP_PATTERN_DTYPE:
            pat[:] = patterns
        else:
            for i, (m, v) in enumerate(patterns):
                pat["mask"][i] = np.frombuffer(bytes(m), np.uint8)
                pat["value"][i] = np.frombuffer(bytes(v), np.uint8)
        return pat

    def set_ft8_ap(self, patterns, max_iter=30, min_nsync=7):
        """cwslg_set_ft8_ap: the a-priori patterns (AP_PATTERN_DTYPE array, or a sequence of (mask[12], value[12]) byte pairs; at most 8, none
        clears them), tried in this order by ap_decode and fetch_ft8_ap.  Host effect only."""
        pat = self._ap_patterns(patterns)
        self._chk(self.L.cwslg_set_ft8_ap(self.h, pat.ctypes.data if len(pat) else None, len(pat), int(max_iter), int(min_nsync)))

    def set_ft4_ap(self, patterns, max_iter=30, min_nsync=8, min_nqual=20):
        """cwslg_set_ft4_ap: the FT4 a-priori patterns, a state of their own beside set_ft8_ap's (FT4's message bits are scrambled on the air: the
        patterns hold the scrambled values).  The same forms of `patterns`; tried in this order by fetch_ft4_ap.  Host effect only."""
        pat = self._ap_patterns(patterns)
        self._chk(self.L.cwslg_set_ft4_ap(self.h, pat.ctypes.data if len(pat) else None, len(pat), int(max_iter), int(min_nsync), int(min_nqual)))

    def fetch_ft4_ap(self, start_epoch=0, max=4096):
        """cwslg_fetch_ft4_ap: the a-priori words of the FT4 group -- the sync records BP and OSD gave up on in every set, each set decoded under the
        patterns of set_ft4_ap, the smallest set with a find chosen, de-duplicated like fetch_decodes.  -> None if no channel takes part, else
        (records, start_epoch, n_total, n_channels): records DECODE_DTYPE with by_osd = 2, set = metric set | pattern << 2 (ap_set_split), dmin =
        OSD's distance of the word.  Words BP / OSD already have are not removed: merge_ap_decodes."""
        buf = np.zeros(int(max) if int(max) > 1 else 1, DECODE_DTYPE)
        t0, n, n_total, n_ch = C.c_uint64(int(start_epoch)), C.c_int(), C.c_int(), C.c_int()
        rc = self.L.cwslg_fetch_ft4_ap(self.h, C.byref(t0), buf.ctypes.data if int(max) > 0 else None, int(max), C.byref(n), C.byref(n_total), C.byref(n_ch))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return buf[:n.value].copy(), t0.value, n_total.value, n_ch.value

    def ap_decode(self, llr):
        """The a-priori kernel on caller-supplied metrics, llr float32[n, 174] (n >= 0), no nsync gate; synchronous.  -> AP_MSG_DTYPE array [n]."""
        llr = np.ascontiguousarray(llr, dtype=np.float32).reshape(-1, 174)
        out = np.zeros(len(llr), AP_MSG_DTYPE)
        self._chk(self.L.cwslg_ap_decode(self.h, llr.ctypes.data if len(llr) else None, len(llr), out.ctypes.data if len(llr) else None))
        return out

    def fetch_ft8_ap(self, start_epoch=0, max=4096):
        """cwslg_fetch_ft8_ap: the a-priori words of the FT8 group -- the entries BP and OSD gave up on, decoded under the patterns of set_ft8_ap,
        chosen and de-duplicated like fetch_decodes.  -> None if no channel takes part, else (records, start_epoch, n_total, n_channels): records
        DECODE_DTYPE with by_osd = 2, set = the pattern index, dmin = OSD's distance of the word.  Words BP / OSD already have are not removed:
        merge_ap_decodes."""
        buf = np.zeros(int(max) if int(max) > 1 else 1, DECODE_DTYPE)
        t0, n, n_total, n_ch = C.c_uint64(int(start_epoch)), C.c_int(), C.c_int(), C.c_int()
        rc = self.L.cwslg_fetch_ft8_ap(self.h, C.byref(t0), buf.ctypes.data if int(max) > 0 else None, int(max), C.byref(n), C.byref(n_total), C.byref(n_ch))
        if rc == ERR_NO_FRAME:
            return None
        self._chk(rc)
        return buf[:n.value].copy(), t0.value, n_total.value, n_ch.value

    def ft4_tones(self, bits):
        """cwslg_ft4_tones: the 103 FT4 channel tones of a 91-bit word (bits[12] as in a decode record; no rvec) under the code in force -> uint8[103]."""
        b = np.ascontiguousarray(np.frombuffer(bytes(bits), np.uint8) if isinstance(bits, (bytes, bytearray)) else np.asarray(bits, np.uint8))
        if b.shape != (12,):
            raise ValueError("bits: 12 bytes")
        tones = np.zeros(103, np.uint8)
        self._chk(self.L.cwslg_ft4_tones(self.h, b.ctypes.data, tones.ctypes.data))
        return tones

    def enable_long_sync(self, on=True, nfa_hz=1400, nfb_hz=1600, minsync=1.2):
        """Candidate search of the 120 s modes (WSPR: wsprd's front end; FST4W-120: get_candidates_fst4 over nfa..nfb)."""
        self._chk(self.L.cwslg_enable_long_sync(self.h, 1 if on else 0, nfa_hz, nfb_hz, minsync))

    def fetch_wspr_candidates(self, ch, max_cand=200, with_epoch=False):
        """-> None until a frame was searched, else [(freq_hz, snr_db, drift, sync, shift)] (with_epoch: (list, frame start epoch))."""
        buf = (WsprCandidate * max_cand)()
        r = self._fetch_records(self.L.cwslg_fetch_wspr_candidates, ch, buf, max_cand)
        if r is None:
            return None
        n, t0 = r
        out = [(b.freq_hz, b.snr_db, b.drift, b.sync, b.shift) for b in buf[:n]]
        return (out, t0) if with_epoch else out

    def fetch_fst4w_candidates(self, ch, max_cand=100, with_epoch=False):
        """-> None until a frame was searched, else [(freq_hz, snr, bin)] (with_epoch: (list, frame start epoch))."""
        buf = (Fst4wCandidate * max_cand)()
        r = self._fetch_records(self.L.cwslg_fetch_fst4w_candidates, ch, buf, max_cand)
        if r is None:
            return None
        n, t0 = r
        out = [(b.freq_hz, b.snr, b.bin) for b in buf[:n]]
        return (out, t0) if with_epoch else out

    def long_sync_debug(self, ch, what):
        """what: 'iq' complex64[46080], 'ps' float32[512, 359] (wsprd's ps[j][i]), 'smspec' float32[411] (WSPR);
        's2' float32[nnw], 'band' complex64[nband] (FST4W)."""
        sel = {"iq": 0, "ps": 1, "smspec": 2, "s2": 3, "band": 4}[what]
        buf = np.empty(2 * 46080 if sel == 0 else (359 * 512 if sel == 1 else (411 if sel == 2 else 65600)), np.float32)
        n = C.c_size_t()
        self._chk(self.L.cwslg_long_sync_debug_fetch(self.h, ch, sel, buf.ctypes.data, buf.nbytes, C.byref(n)))
        out = buf[:n.value]
        if sel in (0, 4):
            return out.view(np.complex64)
        if sel == 1:
            return np.ascontiguousarray(out.reshape(359, 512).T)
        return out

    def set_ft4_syncmin(self, syncmin=1.2):
        self._chk(self.L.cwslg_set_ft4_syncmin(self.h, syncmin))

    def sync_debug(self, ch, what):
        """what: 'spectra' -> float32[steps, row]; 'red'/'red2' -> float32[1921]; 'jpeak'/'jpeak2' -> int32[1921].
        FT4 channels: 'red' = savsm/sbase, 'red2' = sbase (first 1153 entries meaningful)."""
        sel = {"spectra": 0, "red": 1, "red2": 2, "jpeak": 3, "jpeak2": 4, "ft4_cx": 5, "ft4_cd0": 6}[what]
        if sel >= 5:                                    # FT4 coherent stage: complex64[36289] / complex64[4032]
            buf = np.empty(2 * (36289 if sel == 5 else 4032), np.float32)
            n, row = C.c_size_t(), C.c_int()
            self._chk(self.L.cwslg_sync_debug_fetch(self.h, ch, sel, buf.ctypes.data, buf.nbytes, C.byref(n), C.byref(row)))
            return buf.view(np.complex64)
        buf = np.empty(372 * 1936 if sel == 0 else 1921, np.float32 if sel < 3 else np.int32)
        n, row = C.c_size_t(), C.c_int()
        self._chk(self.L.cwslg_sync_debug_fetch(self.h, ch, sel, buf.ctypes.data, buf.nbytes, C.byref(n), C.byref(row)))
        buf = buf[: n.value]
        return buf.reshape(-1, row.value) if sel == 0 else buf

    def stats(self):
        s = Stats()
        self._chk(self.L.cwslg_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in Stats._fields_}

    def reset_stats(self):
        self._chk(self.L.cwslg_reset_stats(self.h))

    def set_timing(self, on=True):
        self._chk(self.L.cwslg_set_timing(self.h, 1 if on else 0))

    def set_scale_factors(self, ft=0.90, wspr=0.20):
        self._chk(self.L.cwslg_set_scale_factors(self.h, ft, wspr))

    def set_exact(self, on=True):
        """Reference-order arithmetic: float and int16 frames bit-identical to the compiled reference."""
        self._chk(self.L.cwslg_set_exact(self.h, 1 if on else 0))

    def demod_kernel_name(self):
        """Name of the kernel the most recent demod launch ran (bench.py's roofline.kernel)."""
        return (self.L.cwslg_demod_kernel_name(self.h) or b"").decode()

    def stream(self):
        return self.L.cwslg_stream(self.h)

    def channel_constants(self, ch):
        """(taps float32[32D], tone complex64[D], phase_inc complex64) exactly as uploaded."""
        D = self.channel_info(ch)["in_size"] // 4
        taps = np.empty(32 * D, np.float32)
        tone = np.empty(2 * D, np.float32)
        inc = np.empty(2, np.float32)
        self._chk(self.L.cwslg_channel_constants(self.h, ch, taps.ctypes.data, tone.ctypes.data, inc.ctypes.data))
        return taps, tone.view(np.complex64), inc.view(np.complex64)[0]

    def checkpoint_stride(self):
        return int(self.L.cwslg_phasor_checkpoint_stride())

    def phasor_checkpoints(self, ch, n=None):
        tot = C.c_size_t()
        self._chk(self.L.cwslg_channel_phasor_checkpoints(self.h, ch, None, 0, C.byref(tot)))
        n = tot.value if n is None else min(n, tot.value)
        out = np.empty(2 * n, np.float32)
        self._chk(self.L.cwslg_channel_phasor_checkpoints(self.h, ch, out.ctypes.data, n, C.byref(tot)))
        return out.view(np.complex64)
