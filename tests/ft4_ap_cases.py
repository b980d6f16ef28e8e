"""Test helper: the two FT4 slots of tests/test_gpu_fetch_ft4_ap.py and, computed on the CPU alone, every stage of their channels: the oracle's
frame, then ft4_softbits_ref, ft4_decode_cases, ft4_osd_cases, ft4_ap_ref and decodes_ref -- tests/ft4_decode_report_cases.py's machinery.
tests/test_ft4_ap_inputs.py proves on that chain what the slots contain.

Each slot is one slot of FT4 IQ at 48 kHz on one receiver, three channels, the third hearing noise alone; messages carry real codewords of
the seed code (no rvec anywhere: the patterns hold the bits as they are on the air).
  "starved"  the boundary runs the FT4 decode with a max_iter so small (STARVED_ITER) that BP fails on most records, OSD off; the a-priori
             patterns are an EMPTY mask -- the plain second pass -- and two known fields, with 30 iterations.  Many finds without a search for
             marginal amplitudes: an addressing error in slot, set or entry cannot hide.  One very strong transmission decodes even so (its
             records are not attempted), one message is sent at two audio frequencies (ndup), weak transmissions under the known fields are
             found only under their pattern or only in a later metric set.
  "normal"   record_race_cases' DECODE4 and OSD4, weak transmissions whose first 29 bits carry a known field: BP and OSD miss some in all
             three sets and the a-priori pass finds them; one that OSD returns is attempted only with OSD off at the boundary."""
import functools

import numpy as np

import ap_cases as APC
import ap_ref as AP
import decodes_ref as DR
import ft4_ap_ref as A4
import ft4_decode_cases as D
import ft4_osd_cases as X
import ft4_softbits_ref as S4
import ldpc_cases as LC
import osd_cases as OC
import record_race_cases as RC

MODE = "FT4"
SEED = APC.SEED
FS, BLK, N_IQ, SIGMA = D.FS, D.BLK, D.N4, D.SIGMA
RF = (9000, -6000, 2000)                    # dial offsets of the three channels; the third hears noise alone
MAX_CAND = 30
SYNCMIN = 1.05                              # cwslg_set_ft4_syncmin: a few noise candidates beside the transmissions, the uncut lists below MAX_CAND
AP_MAX_ITER = 30
STARVED_ITER = 1
SLOTS = ("starved", "normal")
# slot -> (boundary decode settings, boundary OSD settings or None, a-priori minima (min_nsync, min_nqual))
SETTINGS = {"starved": ((STARVED_ITER, X.MIN_NSYNC, X.MIN_NQUAL), None, (9, 21)),
            "normal": (RC.DECODE4, RC.OSD4, (X.MIN_NSYNC, X.MIN_NQUAL))}
P0, P1 = APC.PREFIXES[0], APC.PREFIXES[1]
start_epoch = lambda e: RC.start_epoch(MODE, e)


def patterns(slot, n_pat=None):
    """starved: an empty mask, then the known fields P0 and P1 (n_pat 1: the empty mask alone); normal: P0 and P1 (n_pat 1: P0 alone)."""
    empty = (np.zeros(0, np.uint8), np.zeros(0, np.uint8))
    pairs = [empty, APC.prefix_pattern(P0), APC.prefix_pattern(P1)] if slot == "starved" else [APC.prefix_pattern(P0), APC.prefix_pattern(P1)]
    return AP.make_patterns(pairs[:n_pat])


N_PAT = {"starved": (1, 3), "normal": (1, 2)}


def message(mseed, prefix=None):
    return APC.message(mseed, prefix)


# slot -> channel index -> [(audio Hz of tone 0, start s, amplitude, message seed, known field or None)].  The transmissions sit low in the band:
# a cut FT4 list keeps its FIRST candidates in frequency order.  The weak amplitudes were searched on the CPU chain; what each gives is
# tests/test_ft4_ap_inputs.py's to prove.
LOUD, WEAK = 5000.0, 1120.0
TX = {
    "starved": {0: [(420.0, 0.50, LOUD, 8101, None), (700.0, 0.70, 1500.0, 8102, P0), (980.0, 0.40, 1500.0, 8103, None),
                    (1260.0, 0.60, 1400.0, 8104, P1), (1540.0, 0.30, 1400.0, 8104, P1), (1820.0, 0.80, 1300.0, 8105, P0),
                    (2100.0, 0.45, 1250.0, 8106, P1), (2380.0, 0.65, 1250.0, 8107, P0), (2660.0, 0.35, 1300.0, 8108, P1)],
                1: [(600.0, 0.55, 1700.0, 8111, P1), (1100.0, 0.75, 1300.0, 8112, P0), (1700.0, 0.35, 1200.0, 8113, None),
                    (2300.0, 0.45, 1400.0, 8114, P0)]},
    "normal": {0: [(420.0, 0.50, 1900.0, 8201, None), (700.0, 0.70, WEAK, 8202, P0), (980.0, 0.40, WEAK, 8203, P1),
                   (1260.0, 0.60, WEAK, 8204, P0), (1540.0, 0.30, WEAK, 8205, P1), (1820.0, 0.80, WEAK, 8206, P0),
                   (2100.0, 0.45, WEAK, 8207, P1), (2380.0, 0.65, WEAK, 8208, P0), (2660.0, 0.35, 1200.0, 8209, None)],
               1: [(600.0, 0.55, WEAK, 8211, P1), (1100.0, 0.75, WEAK, 8212, P0), (1700.0, 0.35, 1800.0, 8213, None)]},
}
NOISE_SEED = {"starved": 6161, "normal": 6262}


def sent(slot, k):
    """The 91-bit words channel k was sent, as bits[12] byte strings."""
    return [APC.bits12(message(mseed, pre)) for _, _, _, mseed, pre in TX[slot].get(k, [])]


@functools.lru_cache(maxsize=None)
def slot_iq(slot):
    rng = np.random.default_rng(NOISE_SEED[slot])
    iq = (rng.normal(0.0, SIGMA, N_IQ) + 1j * rng.normal(0.0, SIGMA, N_IQ)).astype(np.complex64)
    for k, txs in TX[slot].items():
        for audio, t0, amp, mseed, pre in txs:
            iq = iq + D.iq_of_tones(N_IQ, RF[k], audio, t0, amp, D.tones_of(LC.encode(SEED, message(mseed, pre))))
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq


def frame_of(iq, k):
    from oracle import oracle as orc
    oc = orc.Channel(MODE, FS, BLK, RF[k])
    assert oc.boundary(start_epoch(0)) is None
    oc.push_many(iq)
    r = oc.boundary(start_epoch(1))
    oc.close()
    assert r is not None and r["t_start"] == start_epoch(0)
    return r["i16"]


def chain_of(fr, max_cand, dec, osd_cfg):
    """Sync, soft, decode and (osd_cfg not None) OSD records of one frame on the CPU."""
    from oracle import oracle as orc
    code, G = LC.make_code(SEED)["code"], OC.generator(SEED)
    cands = orc.ft4_candidates(fr, float(RC.SYNC["f_lo"]), float(RC.SYNC["f_hi"]), SYNCMIN, max_cand)
    recs = orc.ft4_sync_all(fr, cands)
    soft = D.soft_dict(*S4.softbits_of_records(orc, orc.ft4_bigspec(fr), recs))
    msg = D.expected(soft, code, *dec)
    osd = X.expected(soft, msg, G, *osd_cfg) if osd_cfg else None
    return dict(list=cands, sync=recs, soft=soft, msg=msg, osd=osd)


@functools.lru_cache(maxsize=None)
def frame(slot, k):
    return frame_of(slot_iq(slot), k)


@functools.lru_cache(maxsize=None)
def records(slot, k, max_cand=MAX_CAND):
    """Sync records, soft records, decode records and -- where the slot's boundary runs OSD -- OSD records of channel k."""
    dec, osd_cfg, _ = SETTINGS[slot]
    return chain_of(frame(slot, k), max_cand, dec, osd_cfg)


@functools.lru_cache(maxsize=None)
def ap_records(slot, k, max_cand=MAX_CAND, osd=True, n_pat=None):
    """The a-priori records of channel k: osd -- the channel's OSD records are used (a slot whose boundary has OSD off has none to use)."""
    c = records(slot, k, max_cand)
    mins = SETTINGS[slot][2]
    return A4.decode(LC.make_code(SEED)["code"], c["soft"], c["msg"], c["osd"] if osd else None, patterns(slot, n_pat), AP_MAX_ITER, *mins)


def expected(slot, n_chan=3, max_cand=MAX_CAND, osd=True, n_pat=None, max_out=None):
    """What cwslg_fetch_ft4_ap hands out for the slot's first n_chan channels under the ids 0..n_chan - 1."""
    return A4.ap_decodes([(k, DR.where_ft4(records(slot, k, max_cand)["sync"]), ap_records(slot, k, max_cand, osd, n_pat)) for k in range(n_chan)], max_out)


# ---- what a-priori decoding is worth on the FT4 chain: on-frequency transmissions in white noise, the restatements alone -----------------------------
WORTH_AMPS = (1000.0, 1100.0, 1200.0)       # around the level at which this chain's BP + OSD lose the transmissions
WORTH_SEEDS = (0, 1, 2)                     # slots per level
WORTH_HZ = tuple(300.0 + 270.0 * j for j in range(10))      # tone 0 of the ten transmissions of a slot
WORTH_MAX_CAND = 100


def worth_message(level, seed, j):
    return message(30000 + 1000 * level + 10 * seed + j, (P0, P1)[j % 2])


def worth_slot(level, seed):
    """-> (records of channel 0 with the ten transmissions, records of channel 2 with noise alone) under the normal slot's settings."""
    rng = np.random.default_rng(7300 + 10 * level + seed)
    iq = (rng.normal(0.0, SIGMA, N_IQ) + 1j * rng.normal(0.0, SIGMA, N_IQ)).astype(np.complex64)
    for j, hz in enumerate(WORTH_HZ):
        iq = iq + D.iq_of_tones(N_IQ, RF[0], hz, 0.3 + 0.05 * j, WORTH_AMPS[level], D.tones_of(LC.encode(SEED, worth_message(level, seed, j))))
    iq = iq.astype(np.complex64)
    dec, osd_cfg, _ = SETTINGS["normal"]
    return tuple(chain_of(frame_of(iq, k), WORTH_MAX_CAND, dec, osd_cfg) for k in (0, 2))
