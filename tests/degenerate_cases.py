"""Test helper: the inputs of tests/test_gpu_degenerate_frames.py -- what a skimmer hears when it does not hear transmissions in noise: digital
silence, an impulse, unmodulated carriers on and off the bin grid, DC, a carrier that starts in mid-slot, noise-free transmissions, slots whose
IQ stops or starts in the middle, a weak station beside a blocker 40 dB above it, and a comb of carriers -- vetted on the CPU by
tests/test_degenerate_inputs.py.

A recipe is ONE pair slot (softbits_cases.N8 IQ samples at 48 kHz, blocks of 1024) on a receiver of its own, because it defines the whole
wideband IQ (silence means silence).  One FT8 and one FT4 channel sit on that receiver at dial 0: the FT8 channel's frame is the pair slot, the
FT4 channel's frame is the half of it that RECIPES names (0: the first N4 samples, 1: the second).  Transmissions carry codewords of
ldpc_cases.SEEDS[0] (FT8: ldpc_cases.chain_message, FT4: ft4_decode_cases.message), so the 91 bits sent are known.

reference() runs the repository's restatements in order on a frame -- oracle.ft8_spectra / ft8_sync, oracle.ft4_candidates / ft4_sync_all /
ft4_bigspec, ft8_softbits_ref, ft4_softbits_ref, ldpc_ref.hard_records, ft4_decode_cases.expected, osd_ref.chain_records,
ft4_osd_cases.expected -- and returns every stage's output; nothing here restates a kernel.  Two configurations: UPSTREAM (FT8 min_nsync 7, FT4
gates 8 / 20, 30 iterations, OSD order 2) and OPEN (every gate 0, so that every record is attempted and junk goes through BP, OSD and the
harvest).  The list limits are 200 (FT8) and 100 (FT4) in both.

The helpers at the end state the conditions that BOTH the CPU module (on the oracle's own frames) and the GPU module (on the library's output)
assert."""
import collections
import functools
import hashlib

import numpy as np

import decode_reports_ref as RR
import decodes_ref as DR
import ft4_decode_cases as D
import ft4_decode_reports_ref as RR4
import ft4_osd_cases as X
import ft4_softbits_ref as R4
import ft8_softbits_ref as R8
import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O
import report_kernel_cases as K
import softbits_cases as S

FS, BLK, N4, N8, T_HALF = S.FS, S.BLK, S.N4, S.N8, S.T_HALF
U32 = np.uint32
SEED = C.SEEDS[0]
DIAL = 0
F_LO, F_HI, SYNCMIN8, SYNCMIN4 = 200, 3000, 1.5, 1.2
MAX_CAND = {"FT8": 200, "FT4": 100}
IA, IB = 64, 960                                                        # sync8's search bins for 200..3000 Hz
PITCH = R8.soft_pitch(F_HI)

Config = collections.namedtuple("Config", "name max_iter order min_nsync8 min_nsync4 min_nqual4")
UPSTREAM = Config("upstream", 30, 2, 7, 8, 20)
OPEN = Config("open", 30, 2, 0, 0, 0)
CONFIGS = {c.name: c for c in (UPSTREAM, OPEN)}

AMP = 3000.0
CARRIER_HZ, OFF_BIN_HZ = 1500.0, 1501.5625                              # on a bin of both grids (3.125 Hz and 12000 / 2304 Hz share 1500); half an FT8 bin off
CLEAN8 = (1000.0, 0.6, AMP, 1101)                                       # (audio Hz of tone 0, start s, amplitude, message seed)
CLEAN4 = (1000.0, 0.5, AMP, 1102)                                       # start counted from the second half's first sample
BLOCKER_HZ, BLOCKER_AMP = 2000.0, 30000.0
WEAK8 = (800.0, 0.6, 300.0, 1103)
WEAK4 = (800.0, 0.5, 300.0, 1104)
CUT8 = (1000.0, 0.6, AMP, 1105)
CUT4 = (1000.0, 0.5, AMP, 1106)
# Beside CUT4 in both FT4 cut slots.  Five of them begin about 0.3 s BEFORE the FT4 frame: their records have a negative ibest, the symbols before
# sample 0 are exact zeros and so are the LLRs of the data symbols among them -- the only exact zeros an FT4 record can hold, because the zeroed
# stretch of the frame comes back from the frame-long FFT pair of the downsampler as rounding noise, not as zeros.
CUT4_MORE = [(400.0, -0.34, AMP, 1107), (700.0, 0.3, AMP, 1108), (1300.0, -0.30, AMP, 1109), (1600.0, 0.8, AMP, 1110), (1900.0, -0.32, AMP, 1111),
             (2200.0, 0.1, AMP, 1112), (2500.0, -0.33, AMP, 1113), (2800.0, -0.31, AMP, 1114)]
CUT8_TAIL_S, CUT8_HEAD_S, CUT4_S = 6.0, 9.0, 3.0
COMB = [500.0 + 25.0 * k for k in range(80)]
COMB_AMP = 1000.0
IMPULSE_AT, IMPULSE = N4 + 150 * BLK, 20000.0
NOISE_SEEDS = dict(blocker8=1201, blocker4=1202, cut8_tail=1203, cut8_head=1204, cut4_tail=1205, cut4_head=1206)

# name -> the half of the pair slot that is the FT4 channel's frame
RECIPES = dict(zeros=1, impulse=1, dc=1, midslot=0, carrier_on=1, carrier_off=1, comb=1, clean8=1, clean4=1, blocker8=1, blocker4=1,
               cut8_tail=1, cut8_head=1, cut4_tail=1, cut4_head=1)
GROUPS = dict(quiet=("zeros", "impulse", "dc", "midslot"), carriers=("carrier_on", "carrier_off", "comb"),
              clean=("clean8", "clean4", "blocker8", "blocker4"), cut=("cut8_tail", "cut8_head", "cut4_tail", "cut4_head"))
ZERO_FRAMES = (("zeros", "FT8"), ("zeros", "FT4"), ("midslot", "FT4"), ("cut8_tail", "FT4"))      # (recipe, mode) whose frame is all zero


def _carrier(n, hz, amp, first=0):
    return amp * np.exp(2j * np.pi * hz * (np.arange(n) + first) / FS)


def _ft8(tx):
    audio, t0, amp, mseed = tx
    return C.iq_of_tones(FS, N8, DIAL, audio, t0, amp, C.tones_of(C.encode(SEED, C.chain_message(mseed)))).astype(np.complex128)


def _ft4(tx):
    """The transmission in the pair slot, its start counted from the second half's first sample (it may lie a little before it)."""
    audio, t0, amp, mseed = tx
    return D.iq_of_tones(N8, DIAL, audio, T_HALF + t0, amp, D.tones_of(C.encode(SEED, D.message(mseed)))).astype(np.complex128)


@functools.lru_cache(maxsize=None)
def _recipe_iq(name):
    from oracle import oracle as orc
    iq = np.zeros(N8, np.complex128)
    if name in NOISE_SEEDS:
        iq += S.noise_iq(orc, NOISE_SEEDS[name], N8)
    if name == "impulse":
        iq[IMPULSE_AT] = IMPULSE
    elif name == "dc":
        iq += AMP
    elif name == "midslot":
        iq[N4:] = _carrier(N4, CARRIER_HZ, AMP)
    elif name == "carrier_on":
        iq += _carrier(N8, CARRIER_HZ, AMP)
    elif name == "carrier_off":
        iq += _carrier(N8, OFF_BIN_HZ, AMP)
    elif name == "comb":
        for hz in COMB:
            iq += _carrier(N8, hz, COMB_AMP)
    elif name == "clean8":
        iq += _ft8(CLEAN8)
    elif name == "clean4":
        iq += _ft4(CLEAN4)
    elif name == "blocker8":
        iq += _ft8(WEAK8) + _carrier(N8, BLOCKER_HZ, BLOCKER_AMP)
    elif name == "blocker4":
        iq += _ft4(WEAK4) + _carrier(N8, BLOCKER_HZ, BLOCKER_AMP)
    elif name == "cut8_tail":
        iq += _ft8(CUT8)
        iq[int(CUT8_TAIL_S * FS):] = 0
    elif name == "cut8_head":
        iq += _ft8(CUT8)
        iq[:int(CUT8_HEAD_S * FS)] = 0
    elif name == "cut4_tail":
        iq += _ft4(CUT4) + sum(_ft4(tx) for tx in CUT4_MORE)
        iq[N4 + int(CUT4_S * FS):] = 0
    elif name == "cut4_head":
        iq += _ft4(CUT4) + sum(_ft4(tx) for tx in CUT4_MORE)
        iq[N4:N4 + int(CUT4_S * FS)] = 0
    else:
        assert name == "zeros", name
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq


def recipe_iq(name):
    """complex64[N8], read-only: the pair slot of a recipe."""
    assert name in RECIPES, name
    return _recipe_iq(name)


# ---- the ordinary slot before and after ------------------------------------------------------------------------------------------------------------
ORDINARY_SEED = 1300
ORDINARY8 = [(812.5, 0.64, 3000.0, 1301), (2437.5, 1.20, 2500.0, 1302)]   # softbits_cases bursts: (audio Hz, start s, amplitude, tone seed)
ORDINARY4 = [(700.0, 0.40, 3000.0, 1303), (1600.0, 0.75, 2800.0, 1304)]


@functools.lru_cache(maxsize=None)
def ordinary():
    """-> (iq complex64[N8], tones): noise that fills the pair slot, two FT8 bursts and, in the second half, two FT4 bursts; every channel of
    every receiver hears all of them (one dial)."""
    from oracle import oracle as orc
    iq, tones = S.pair_iq(orc, ORDINARY_SEED, [(DIAL, ORDINARY8)], [(DIAL, ORDINARY4)])
    iq.setflags(write=False)
    return iq, tones


# ---- frames ----------------------------------------------------------------------------------------------------------------------------------------
def oracle_frame(oracle, mode, iq, half=1):
    """The int16 frame oracle.Channel makes of a pair slot: FT8 the whole of it, FT4 the named half."""
    if mode == "FT8":
        return S.oracle_frame(oracle, "FT8", DIAL, iq)
    if half == 0:
        return S.oracle_frame(oracle, "FT4", DIAL, iq[:N4])
    return S.oracle_frame(oracle, "FT4", DIAL, iq, split=N4)


@functools.lru_cache(maxsize=None)
def recipe_frame(name, mode):
    from oracle import oracle as orc
    fr = oracle_frame(orc, mode, recipe_iq(name), RECIPES[name])
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def ordinary_frame(mode):
    from oracle import oracle as orc
    fr = oracle_frame(orc, mode, ordinary()[0], 1)
    fr.setflags(write=False)
    return fr


# ---- every stage of the restatement ------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def reference(oracle, mode, i16, config, max_cand=None):
    """Every stage's output for one int16 frame under `config`, each stage fed the one before; computed once per (mode, frame, config, limit) and
    shared (the arrays are read-only).  FT8: plane, arrays (red, red2, jpeak, jpeak2), list, llr, sigma, nsync, msg, osd.  FT4: arrays (savsm,
    sbase), list, cx, recs, llr, sigma, nsync, nqual, msg, osd."""
    i16 = np.ascontiguousarray(i16, np.int16)
    max_cand = MAX_CAND[mode] if max_cand is None else max_cand
    key = (mode, hashlib.sha1(i16.tobytes()).hexdigest(), config, max_cand)
    if key in _CACHE:
        return _CACHE[key]
    code, G = C.make_code(SEED)["code"], OC.generator(SEED)
    if mode == "FT8":
        plane = np.ascontiguousarray(oracle.ft8_spectra(i16, PITCH), np.float32)
        cands, arrays = oracle.ft8_sync(i16, F_LO, F_HI, SYNCMIN8, max_cand, want_arrays=True)
        llr, sigma, nsync = R8.softbits(plane, cands)
        msg = R.hard_records(code, llr, config.max_iter, nsync, sigma, config.min_nsync8)
        osd = O.chain_records(G, llr, config.order, nsync, msg, config.min_nsync8)
        out = dict(frame=i16, plane=plane, arrays=arrays, list=cands, llr=llr, sigma=sigma, nsync=nsync, msg=msg, osd=osd)
    else:
        cands, arrays = oracle.ft4_candidates(i16, float(F_LO), float(F_HI), SYNCMIN4, max_cand, want_arrays=True)
        recs = oracle.ft4_sync_all(i16, cands)
        cx = oracle.ft4_bigspec(i16)
        soft = D.soft_dict(*R4.softbits_of_records(oracle, cx, recs))
        msg = D.expected(soft, code, config.max_iter, config.min_nsync4, config.min_nqual4)
        osd = X.expected(soft, msg, G, config.order, config.min_nsync4, config.min_nqual4)
        out = dict(frame=i16, arrays=arrays, list=cands, cx=cx, recs=recs, msg=msg, osd=osd, **soft)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CACHE[key] = out
    return out


def stage_floats(ref):
    """name -> every floating-point output of a reference() result, for the NaN / infinity check."""
    out = {k: np.asarray(v) for k, v in ref.items() if isinstance(v, np.ndarray) and v.dtype.kind in "fc"}
    out.update({k: np.asarray(v) for k, v in ref["arrays"].items() if v.dtype.kind == "f"})
    out["list"] = np.array([c[2:] for c in ref["list"]], np.float64).reshape(-1)
    if "recs" in ref:
        out["recs"] = np.array([[h[n] for n in ("f0_hz", "f1_hz", "dt_s", "sync")] for h in ref["recs"]], np.float64).reshape(-1)
    osd = ref["osd"]
    out["dmin"] = np.asarray(osd["set"]["dmin"] if "set" in osd.dtype.names else osd["dmin"]).reshape(-1)
    return out


# The one place where the restatements leave the finite numbers: getcandidates4's baseline of an ALL-ZERO frame.  10 log10(0) is -inf in
# float32, the polynomial fitted through it is NaN, `sbase > 0` fails and the search ends without a candidate; sbase[nfa..nfb] keeps the NaN.
# There the comparison follows tests/test_gpu_longsync_edges.py: NaN where the restatement has NaN, of any sign and payload; all else on bits.
NAN_ALLOWED = {(name, mode, "sbase") for name, mode in ZERO_FRAMES if mode == "FT4"}


def same_bits(got, want):
    """got == want as bit patterns, except that a NaN of `want` is matched by any NaN."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype == np.complex64:
        got, want = got.view(np.float32), want.view(np.float32)
    assert got.dtype == np.float32, got.dtype
    nan = np.isnan(want)
    return bool(np.array_equal(nan, np.isnan(got)) and np.array_equal(got.view(U32)[~nan], want.view(U32)[~nan]))


def decodes_of(mode, ch_id, ref, osd=True):
    """decodes_ref's input of one channel from a reference() result or from the GPU's fetches arranged like one."""
    where = DR.where_ft8(ref["list"]) if mode == "FT8" else DR.where_ft4(ref["recs"])
    return ch_id, where, ref["msg"], ref["osd"] if osd else None


def reports_of(planes, lists, dec):
    """decode_reports_ref.reports under the seed code."""
    return RR.reports(K.encoder(SEED), planes, lists, dec)


def reports4_of(spectra, records, dec):
    """ft4_decode_reports_ref.reports under the seed code: spectra[ch_id] the frame spectrum (ft4_cx), records[ch_id] the sync records."""
    from oracle import oracle as orc
    return RR4.reports(orc, K.encoder(SEED), spectra, records, dec)


def ft4_reports(ref, osd=True):
    """(decodes, reports) of ONE FT4 channel (ch_id 0) from a reference() result: what cwslg_fetch_ft4_decode_reports hands out for it."""
    dec, _ = DR.decodes("FT4", [decodes_of("FT4", 0, ref, osd)])
    return dec, reports4_of({0: ref["cx"]}, {0: ref["recs"]}, dec)


# ---- the conditions -------------------------------------------------------------------------------------------------------------------------------------
def bits12(mode, tx):
    """bits[12] of a record that carries the message of transmission tx."""
    m = C.chain_message(tx[3]) if mode == "FT8" else D.message(tx[3])
    return np.packbits(np.concatenate([m, np.zeros(5, np.uint8)])).tobytes()


def words(mode, msg, osd):
    """[(entry, by_osd, bits)] of the entries that carry a word, all-zero words included: the word rule of decodes_ref without its zero rule."""
    out = []
    for q in range(len(msg)):
        w = (DR._word_ft8 if mode == "FT8" else DR._word_ft4)(msg[q], None if osd is None else osd[q])
        if w is not None:
            out.append((q, w[0], w[2]))
    return out


def zero_words(mode, msg, osd):
    """The entries whose word is the all-zero word (crc_ok holds for it: the CRC-14 of 77 zeros is zero)."""
    return [q for q, _, b in words(mode, msg, osd) if DR.all_zero_word(b)]


def duplicates(values):
    """How many of the float32 values repeat an earlier one's bit pattern."""
    v = np.ascontiguousarray(values, np.float32).view(U32)
    return int(v.size - np.unique(v).size)


def exact_zero_llrs(llr):
    return int((np.asarray(llr) == 0).sum())


def segments(recs):
    return {int(h["seg"]) for h in recs}


def assert_sent_ft8(ref, tx):
    """The strongest list entry decodes the message sent, with nsync 21; -> its index."""
    assert ref["list"], "empty list"
    q = int(np.argmax([c[2] for c in ref["list"]]))
    rec = ref["msg"][q]
    assert ref["nsync"][q] == 21 and rec["crc_ok"] and bytes(bytearray(rec["bits"])) == bits12("FT8", tx), (q, int(ref["nsync"][q]), rec)
    return q


def assert_sent_ft4(ref, tx):
    """The strongest sync record decodes the message sent, with nsync 16; -> its index."""
    assert ref["recs"], "no sync record"
    q = int(np.argmax([h["sync"] for h in ref["recs"]]))
    b, by_osd = X.word_bits(ref["msg"], ref["osd"], q)
    assert ref["nsync"][q] == 16 and b is not None and R.pack_bits(b).tobytes() == bits12("FT4", tx), (q, int(ref["nsync"][q]), ref["recs"][q])
    return q


def assert_decoded(mode, ref, tx):
    """Some entry carries the message sent (the blocker recipes: the weak station need not be the strongest entry)."""
    want = bits12(mode, tx)
    hit = [q for q, _, b in words(mode, ref["msg"], ref["osd"]) if b == want]
    assert hit, ("message not decoded", mode, tx, len(ref["msg"]))
    return hit


def assert_conditions(name, mode, cfg, ref, fast_frame=False):
    """What recipe `name` must put before the kernels, on the channel of `mode` under configuration `cfg`.  The floors sit well under what the
    restatements give on the oracle's frames (tests/test_degenerate_inputs.py lists them); the frames are deterministic: a floor that fails means
    the recipe changes, not the floor.  fast_frame: `ref` was made of a fast-mode frame, which may differ from the oracle's by 1 LSB per sample;
    ONE condition is then not asserted -- blocker8's "max |llr| above 1000": that maximum belongs to ONE junk candidate beside the blocker (9332 on the
    oracle's frame, the next candidate's maximum is 13.3) and single LSBs of the frame decide it: the oracle's frame with a random -1, 0 or +1 on
    every sample gives 13.3, 6599 or 4666 (three draws), the fast mode's frame gave 13.3 on an MI355X (tests/test_gpu_degenerate_frames.py
    prints it).  The LLRs themselves are still compared on bits with the restatement of that frame, and every
    other condition holds in both modes."""
    fr, lst = ref["frame"], ref["list"]
    is_open = cfg.name == "open"
    if (name, mode) in ZERO_FRAMES:
        assert not fr.any() and lst == []
    elif name == "impulse":
        assert 1 <= np.count_nonzero(fr) <= 64 and lst == []
    elif name == "carrier_on" and mode == "FT8":
        assert len(lst) == 200
        assert duplicates(ref["arrays"]["red"][IA:IB + 1]) >= 100
        assert ref["sigma"].min() < 0.01 and ref["sigma"].max() > 1e4, (ref["sigma"].min(), ref["sigma"].max())
        if is_open:
            assert len(zero_words("FT8", ref["msg"], ref["osd"])) >= 1
    elif name == "carrier_on":
        assert max(c[2] for c in lst) > 1e10 and segments(ref["recs"]) == {1, 2, 3}, (lst[:3], segments(ref["recs"]))
    elif name == "carrier_off":
        assert lst == [] if mode == "FT8" else len(ref["recs"]) >= 3
    elif name == "dc":
        assert fr.max() == 0 and fr.min() < 0
        assert len(lst) >= 200 if mode == "FT8" else lst == []
    elif name == "midslot":
        assert len(lst) == 200
    elif name == "clean8" and mode == "FT8":
        q = assert_sent_ft8(ref, CLEAN8)
        assert exact_zero_llrs(ref["llr"]) >= 100
        dec, _ = DR.decodes("FT8", [decodes_of("FT8", 0, ref)])
        rep = reports_of({0: ref["plane"]}, {0: ref["list"]}, dec)
        at = [p for p in range(len(dec)) if bytes(bytearray(dec["bits"][p])) == bits12("FT8", CLEAN8)]
        assert len(at) == 1 and dec["entry"][at[0]] == q and rep["snr_db"][at[0]] > 25, (dec, rep)
    elif name == "clean4" and mode == "FT4":
        assert_sent_ft4(ref, CLEAN4)
    elif name in ("cut8_tail", "cut8_head") and mode == "FT8":
        assert exact_zero_llrs(ref["llr"]) >= 5000
    elif name in ("cut4_tail", "cut4_head") and mode == "FT4":
        assert exact_zero_llrs(ref["llr"]) >= 30 and segments(ref["recs"]) == {1, 2, 3}
    elif name == "blocker8" and mode == "FT8":
        assert fast_frame or np.abs(ref["llr"]).max() > 1000
        assert_decoded("FT8", ref, WEAK8)
    elif name == "blocker4" and mode == "FT4":
        assert_decoded("FT4", ref, WEAK4)
    elif name == "comb" and mode == "FT4" and is_open:
        zeros = zero_words("FT4", ref["msg"], ref["osd"])
        assert len(ref["recs"]) >= 100 and len(zeros) >= 50, (len(ref["recs"]), len(zeros))
        dec, _ = DR.decodes("FT4", [decodes_of("FT4", 0, ref)])
        assert not set(int(e) for e in dec["entry"]) & set(zeros) and not any(DR.all_zero_word(b) for b in dec["bits"])


def assert_ordinary(mode, ref, tones):
    """Every burst of the ordinary slot is found with a full nsync and no wrong sign (softbits_cases' condition)."""
    if mode == "FT8":
        S.assert_ft8_found(ref["list"], ref["llr"], ref["nsync"], ORDINARY8, tones[("FT8", DIAL)])
    else:
        S.assert_ft4_found(ref["recs"], ref["llr"], ref["nsync"], ORDINARY4, tones[("FT4", DIAL)])
