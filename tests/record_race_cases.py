"""Test helper: the inputs of tests/test_gpu_record_fetch_races.py -- a sequence of DISTINCT slots per mode (FT8 and FT4, 48 kHz, two channels
each, transmissions that carry codewords of the first seed code of tests/ldpc_cases.py) -- and expected(): what every fetch of the decode chain
must hand out for a channel, an epoch and the configuration in force at that epoch's boundary, computed on the CPU alone from the restatements
(oracle.Channel -> oracle.ft8_sync / ft4_candidates -> oracle.ft4_sync_all -> ft8_softbits_ref / ft4_softbits_ref -> ldpc_ref -> osd_ref), as
byte strings in the layout of the C records.  tests/test_record_race_inputs.py vets the slots: any two epochs differ in every stage, so a stale
or a mixed generation is always visible.  If a property is missing there the amplitudes below change, not the assertions.
group_expected() does the same for the group fetches of tests/test_gpu_report_fetch_races.py: the decodes and the signal reports of a whole
group and epoch (decodes_ref, decode_reports_ref, ft4_decode_reports_ref on the same CPU chain)."""
import collections
import functools

import numpy as np

import ft4_decode_cases as D
import ft4_osd_cases as X
import ft4_softbits_ref as S4
import ft8_softbits_ref as S8
import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O

SEED = C.SEEDS[0]
FS = OC.CHAIN_FS
MODES = ("FT8", "FT4")
BLK = {"FT8": OC.CHAIN_BLK, "FT4": D.BLK}
N_IQ = {"FT8": OC.CHAIN_N, "FT4": D.N4}                                 # one slot of IQ
SIGMA = {"FT8": OC.CHAIN_SIGMA, "FT4": D.SIGMA}
RF = {"FT8": (OC.CHAIN[0][0], OC.CHAIN[2][0]), "FT4": (X.RF_TX, X.RF_NOISE)}      # two dial offsets per mode
PERIOD = {"FT8": 15, "FT4": 7}
FIRST = {"FT8": 1, "FT4": 10}                                           # the epoch of the first boundary, which discards its partial slot
# The free-running tests use the first 5 FT8 and 6 FT4 epochs; the toggle schedules (one step per EMITTING boundary, so that every step frees or
# reallocates arrays that hold a previous epoch's records) have 6 and 7 steps and use one epoch more.
N_RACE = {"FT8": 5, "FT4": 6}
N_EPOCHS = {"FT8": 6, "FT4": 7}
MAX_CAND, CUT_CAND = 12, 5
SYNC = OC.CHAIN_SYNC
SYNCMIN_FT4 = 1.10                                                      # cwslg_set_ft4_syncmin
DECODE8 = (OC.CHAIN_MAX_ITER, OC.CHAIN_MIN_NSYNC)                       # cwslg_enable_ft8_decode
OSD8 = (OC.CHAIN_ORDER, OC.CHAIN_OSD_MIN_NSYNC)                         # cwslg_enable_ft8_osd: order 2
DECODE4 = (X.MAX_ITER, X.MIN_NSYNC, X.MIN_NQUAL)                        # cwslg_enable_ft4_decode
OSD4 = (X.ORDER, X.MIN_NSYNC, X.MIN_NQUAL)                              # cwslg_enable_ft4_osd: order 2

# What is in force at a boundary: the list limit and which stages run (coherent: the FT4 refinement; FT8 ignores it).  A stage runs only with
# the ones before it: soft bits need the coherent stage (FT4), the decode needs soft bits, OSD needs the decode.
Config = collections.namedtuple("Config", "max_cand soft decode osd coherent")
ALL_ON = Config(MAX_CAND, True, True, True, True)
# The toggle test's schedules, one step per emitting boundary: config_at(mode, e) is in force at the boundary that ends epoch e.  Every step
# frees or reallocates record arrays that hold the previous epoch's records.
SCHEDULE = {"FT8": (ALL_ON, ALL_ON._replace(osd=False), ALL_ON._replace(decode=False), ALL_ON, ALL_ON._replace(max_cand=CUT_CAND), ALL_ON),
            "FT4": (ALL_ON, ALL_ON._replace(osd=False), ALL_ON._replace(decode=False), ALL_ON, ALL_ON._replace(coherent=False),
                    ALL_ON._replace(max_cand=CUT_CAND), ALL_ON)}
assert all(len(SCHEDULE[m]) == N_EPOCHS[m] for m in MODES)
STAGES = {"FT8": ("frame", "list", "soft", "msg", "osd"), "FT4": ("frame", "list", "sync", "soft", "msg", "osd")}

CAND_DTYPE = np.dtype([("freq_bin", np.int32), ("time_step", np.int32), ("sync", np.float32), ("freq_hz", np.float32), ("dt_s", np.float32)])
SYNC4_DTYPE = np.dtype([("f0_hz", np.float32), ("f1_hz", np.float32), ("dt_s", np.float32), ("sync", np.float32), ("ibest", np.int32),
                        ("idf", np.int32), ("seg", np.int32), ("cand", np.int32)])
# bytes per record of each stage's byte string (the frame is one record)
RECORD_BYTES = {"list": CAND_DTYPE.itemsize, "sync": SYNC4_DTYPE.itemsize, ("FT8", "soft"): 4 * 176, ("FT4", "soft"): 4 * 527,
                ("FT8", "msg"): R.MSG_DTYPE.itemsize, ("FT4", "msg"): D.MSG4_DTYPE.itemsize, ("FT8", "osd"): O.OSD_DTYPE.itemsize,
                ("FT4", "osd"): X.OSD4_DTYPE.itemsize}


def start_epoch(mode, e):
    """The start epoch the library stamps on the results of epoch index e (the boundary that ends it carries start_epoch(mode, e + 1))."""
    return FIRST[mode] + PERIOD[mode] * e


def epoch_index(mode, t):
    e, rest = divmod(int(t) - FIRST[mode], PERIOD[mode])
    return e if rest == 0 and 0 <= e < N_EPOCHS[mode] else None


# ---- the slots ----------------------------------------------------------------------------------------------------------------------------------
# Per epoch and channel a strong transmission, which belief propagation decodes (its OSD record is not attempted), and a weak one -- in the range
# of osd_cases.CHAIN_RECOVERED's amplitudes (FT8) and of ft4_osd_cases.RECIPES' scaled "small" recipe (FT4) -- which belief propagation fails on,
# so that OSD attempts it and, in the epochs and channels RECOVERED names, returns it with crc_ok and the bits sent.  Message seeds, audio
# frequencies, start times and amplitudes are the epoch's own.  FT8 tones sit on the search grid (3.125 Hz, 40 ms).  The FT4 bursts sit low in
# the band, because a cut FT4 list keeps its FIRST candidates in frequency order, and three more bursts per channel higher up lengthen the
# lists; SYNCMIN_FT4 leaves a few noise candidates beside them, so that every uncut list is longer than CUT_CAND and every list has records that
# fail the gates.  The weak amplitudes were searched on the CPU with the restatements; tests/test_record_race_inputs.py proves what they do.
WEAK = {"FT8": 800.0, "FT4": 1200.0}
RECOVERED = {"FT8": ((1, 0), (2, 0), (3, 0)),                            # (epoch index, channel index): OSD returns the weak transmission where BP failed
             "FT4": ((0, 0), (2, 0), (3, 0), (4, 0), (5, 0), (5, 1))}


def transmissions(mode, e, k):
    """[(audio Hz of tone 0, start s, amplitude, message seed)] of channel k in epoch e: the strong one, the weak one, then (FT4) the three others."""
    if mode == "FT8":
        return [(3.125 * (160 + 24 * e + 8 * k), 0.04 * (5 + 3 * e + k), 1300.0 + 20.0 * e, 500 + 10 * e + 2 * k),
                (3.125 * (480 + 40 * e + 16 * k), 0.04 * (22 - 2 * e + k), WEAK[mode], 501 + 10 * e + 2 * k)]
    return [(300.0 + 60.0 * e + 25.0 * k, 0.80 - 0.06 * e + 0.03 * k, 1600.0 + 30.0 * e, 600 + 10 * e + 2 * k),
            (800.0 + 45.0 * e + 20.0 * k, 0.35 + 0.05 * e + 0.02 * k, WEAK[mode], 601 + 10 * e + 2 * k)] + [
            (1400.0 + 500.0 * j + 40.0 * e + 15.0 * k, 0.30 + 0.20 * j + 0.04 * e, 1500.0, 700 + 10 * e + 3 * k + j) for j in range(3)]


def message(mseed):
    return C.chain_message(mseed)


@functools.lru_cache(maxsize=None)
def slot_iq(mode, e):
    """The slot of IQ (complex64, read-only) of epoch e: noise of the epoch's own seed and both channels' transmissions."""
    n, sigma = N_IQ[mode], SIGMA[mode]
    rng = np.random.default_rng(9000 + 100 * MODES.index(mode) + e)
    iq = (rng.normal(0.0, sigma, n) + 1j * rng.normal(0.0, sigma, n)).astype(np.complex64)
    for k, rf in enumerate(RF[mode]):
        for audio, t0, amp, mseed in transmissions(mode, e, k):
            cw = C.encode(SEED, message(mseed))
            if mode == "FT8":
                iq = iq + C.iq_of_tones(FS, n, rf, audio, t0, amp, C.tones_of(cw))
            else:
                iq = iq + D.iq_of_tones(n, rf, audio, t0, amp, D.tones_of(cw))
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq


# ---- byte strings in the layout of the C records ------------------------------------------------------------------------------------------------
def list_bytes(cands):
    """A candidate list (tuples as fetch_candidates and the oracle return them) as cwslg_candidate records."""
    return np.array([tuple(c) for c in cands], CAND_DTYPE).tobytes()


def sync_bytes(recs):
    """FT4 sync records (dicts as fetch_ft4_sync and oracle.ft4_sync_all return them) as cwslg_ft4_sync records."""
    return np.array([tuple(r[n] for n in SYNC4_DTYPE.names) for r in recs], SYNC4_DTYPE).tobytes()


def soft8_bytes(llr, sigma, nsync):
    """cwslg_ft8_soft records: 174 metrics, sigma, nsync."""
    llr = np.ascontiguousarray(llr, np.float32).reshape(-1, 174)
    cols = [llr.view(np.uint32), np.asarray(sigma, np.float32).reshape(-1, 1).view(np.uint32), np.asarray(nsync).astype(np.int32).reshape(-1, 1).view(np.uint32)]
    return np.ascontiguousarray(np.concatenate(cols, axis=1)).tobytes()


def soft4_bytes(llr, sigma, nsync, nqual):
    """cwslg_ft4_soft records without their padding word: 3 x 174 metrics, 3 sigmas, nsync, nqual."""
    llr = np.ascontiguousarray(llr, np.float32).reshape(-1, 522)
    cols = [llr.view(np.uint32), np.ascontiguousarray(sigma, np.float32).reshape(-1, 3).view(np.uint32),
            np.asarray(nsync).astype(np.int32).reshape(-1, 1).view(np.uint32), np.asarray(nqual).astype(np.int32).reshape(-1, 1).view(np.uint32)]
    return np.ascontiguousarray(np.concatenate(cols, axis=1)).tobytes()


def record_bytes(mode, stage):
    return RECORD_BYTES.get(stage) or RECORD_BYTES[(mode, stage)]


def first_difference(mode, stage, got, want):
    """'' if the byte strings are equal, else a description: the counts, the index of the first differing record and both records."""
    if got == want:
        return ""
    if stage == "frame":
        a, b = np.frombuffer(got, np.int16), np.frombuffer(want, np.int16)
        if len(a) != len(b):
            return f"{len(a)} samples, expected {len(b)}"
        i = int(np.nonzero(a != b)[0][0])
        return f"first differing sample {i}: {int(a[i])}, expected {int(b[i])}"
    rb = record_bytes(mode, stage)
    na, nb = len(got) // rb, len(want) // rb
    for q in range(min(na, nb)):
        if got[q * rb:(q + 1) * rb] != want[q * rb:(q + 1) * rb]:
            return f"{na} records, expected {nb}; first differing record {q}: {got[q * rb:(q + 1) * rb][:24].hex()}..., expected {want[q * rb:(q + 1) * rb][:24].hex()}..."
    return f"{na} records, expected {nb}"


# ---- expected values ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames(mode, k):
    """The oracle's int16 frame of every epoch of channel k (read-only): the channel driven as the tests drive the library -- a first boundary
    that discards, then a slot of IQ and a boundary per epoch."""
    from oracle import oracle as orc
    oc = orc.Channel(mode, FS, BLK[mode], RF[mode][k])
    assert oc.boundary(start_epoch(mode, 0)) is None
    out = []
    for e in range(N_EPOCHS[mode]):
        oc.push_many(slot_iq(mode, e))
        r = oc.boundary(start_epoch(mode, e + 1))
        assert r is not None and r["t_start"] == start_epoch(mode, e)
        r["i16"].setflags(write=False)
        out.append(r["i16"])
    oc.close()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def chain(mode, k, e, max_cand):
    """Every stage of channel k in epoch e with the list limit max_cand and everything on: dict(frame, list, [sync,] soft, msg, osd) of arrays
    and lists as the restatements return them; uncut: the length of the list without a limit that matters (200)."""
    from oracle import oracle as orc
    fr = frames(mode, k)[e]
    code, G = C.make_code(SEED)["code"], OC.generator(SEED)
    if mode == "FT8":
        cands = orc.ft8_sync(fr, SYNC["f_lo"], SYNC["f_hi"], SYNC["syncmin"], max_cand)
        llr, sigma, nsync = S8.softbits(orc.ft8_spectra(fr, S8.soft_pitch(SYNC["f_hi"])), cands)
        msg = R.hard_records(code, llr, DECODE8[0], nsync, sigma, DECODE8[1])
        osd = O.chain_records(G, llr, OSD8[0], nsync, msg, OSD8[1])
        return dict(frame=fr, list=cands, soft=(llr, sigma, nsync), msg=msg, osd=osd)
    cands = orc.ft4_candidates(fr, float(SYNC["f_lo"]), float(SYNC["f_hi"]), SYNCMIN_FT4, max_cand)
    recs = orc.ft4_sync_all(fr, cands)
    soft = D.soft_dict(*S4.softbits_of_records(orc, orc.ft4_bigspec(fr), recs))
    msg = D.expected(soft, code, *DECODE4)
    osd = X.expected(soft, msg, G, *OSD4)
    return dict(frame=fr, list=cands, sync=recs, soft=soft, msg=msg, osd=osd)


def uncut_list_length(mode, k, e):
    from oracle import oracle as orc
    fr = frames(mode, k)[e]
    if mode == "FT8":
        return len(orc.ft8_sync(fr, SYNC["f_lo"], SYNC["f_hi"], SYNC["syncmin"], 200))
    return len(orc.ft4_candidates(fr, float(SYNC["f_lo"]), float(SYNC["f_hi"]), SYNCMIN_FT4, 200))


@functools.lru_cache(maxsize=None)
def expected(mode, k, e, cfg=ALL_ON):
    """What the fetches of channel index k hand out under start_epoch(mode, e) when `cfg` was in force at that epoch's boundary: dict stage ->
    byte string in the C records' layout ("frame": the int16 frame), None for a stage that did not run -- nothing of it may then come back
    stamped with that epoch."""
    c = chain(mode, k, e, cfg.max_cand)
    out = dict(frame=c["frame"].tobytes(), list=list_bytes(c["list"]))
    soft = cfg.soft and (mode == "FT8" or cfg.coherent)
    if mode == "FT8":
        out["soft"] = soft8_bytes(*c["soft"]) if soft else None
    else:
        out["sync"] = sync_bytes(c["sync"]) if cfg.coherent else None
        s = c["soft"]
        out["soft"] = soft4_bytes(s["llr"], s["sigma"], s["nsync"], s["nqual"]) if soft else None
    out["msg"] = c["msg"].tobytes() if soft and cfg.decode else None
    out["osd"] = c["osd"].tobytes() if soft and cfg.decode and cfg.osd else None
    assert set(out) == set(STAGES[mode])
    return out


# ---- the group fetches ------------------------------------------------------------------------------------------------------------------------------
def chain_runs(mode, cfg):
    """The whole chain up to the decode ran at a boundary under cfg: only then do the group fetches hand anything out under that epoch."""
    return bool(cfg.soft and cfg.decode and (mode == "FT8" or cfg.coherent))


@functools.lru_cache(maxsize=None)
def _group(mode, e, max_cand, osd):
    """(decodes, reports) of epoch e with the channel INDEX in ch_id; read-only."""
    from oracle import oracle as orc
    import decode_reports_ref as RR8
    import decodes_ref as DR
    import ft4_decode_reports_ref as RR4
    import report_kernel_cases as K
    chains = [chain(mode, k, e, max_cand) for k in range(len(RF[mode]))]
    inp = [(k, DR.where_ft8(c["list"]) if mode == "FT8" else DR.where_ft4(c["sync"]), c["msg"], c["osd"] if osd else None) for k, c in enumerate(chains)]
    dec, n_total = DR.decodes(mode, inp)
    assert n_total == len(dec)
    enc = K.encoder(SEED)
    if mode == "FT8":
        planes = {k: np.ascontiguousarray(orc.ft8_spectra(c["frame"], S8.soft_pitch(SYNC["f_hi"])), np.float32) for k, c in enumerate(chains)}
        rep = RR8.reports(enc, planes, {k: c["list"] for k, c in enumerate(chains)}, dec)
    else:
        rep = RR4.reports(orc, enc, {k: orc.ft4_bigspec(c["frame"]) for k, c in enumerate(chains)}, {k: c["sync"] for k, c in enumerate(chains)}, dec)
    dec.setflags(write=False)
    rep.setflags(write=False)
    return dec, rep


def group_expected(mode, e, cfg, ch_ids):
    """What cwslg_fetch_decodes and the mode's report fetch hand out for the whole group under start_epoch(mode, e) when `cfg` was in force at
    that epoch's boundary, computed on the CPU alone: (decodes DECODE_DTYPE[n_total], reports REPORT_DTYPE[n_total], n_total) -- decodes_ref on
    chain() of every channel (OSD records only if cfg.osd), decode_reports_ref on the oracle's symbol-spectra planes and the lists (FT8),
    ft4_decode_reports_ref on the oracle's frame spectra and the sync records (FT4), under the encoder of the seed code.  ch_ids: the library's
    channel ids in the order of RF[mode], ascending.  None where the chain did not run at that boundary: the group fetches then hand out nothing
    stamped with that epoch.  A caller that asked with `max` compares against the first min(n_total, max) of both."""
    if not chain_runs(mode, cfg):
        return None
    ch_ids = [int(c) for c in ch_ids]
    assert len(ch_ids) == len(RF[mode]) and ch_ids == sorted(ch_ids), ch_ids
    dec, rep = _group(mode, e, cfg.max_cand, bool(cfg.osd))
    dec = dec.copy()
    dec["ch_id"] = np.asarray(ch_ids, np.int32)[dec["ch_id"]]
    dec.setflags(write=False)
    return dec, rep, len(dec)
