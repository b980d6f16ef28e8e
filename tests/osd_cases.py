"""Test helper: the metric sets the OSD tests share, under the two test codes of tests/ldpc_cases.py, with the restatement's records computed once
(tests/test_osd_cases_inputs.py checks with the restatement alone what each set is FOR), and the chain case."""
import functools

import numpy as np

import ldpc_cases as C
import ldpc_ref as R
import osd_ref as O

F32 = np.float32
N, K = O.N, O.K
SEEDS = C.SEEDS
ORDERS = (0, 1, 2)
BATCHES = (0, 1, 3, 4, 5, 9)                # empty, one wave, a partial and a full workgroup, the step into the next, three workgroups
NOISE = 0.85                                # the noisy codewords: llr = 2.83 (s + 0.85 N(0, 1)); belief propagation (30 iterations) fails on the chosen ones
# per code: the noise seeds of "h1" (OSD returns the sent word with one flip), "h2" (with two), "o2" (another one that order 1 gets wrong and order
# 2 right), found by search with the restatement; the inputs test proves each
NOISY = {1741: dict(h1=100, h2=110, o2=113), 9183: dict(h1=106, h2=103, o2=109)}
NAMES = ("clean", "h1", "h2", "o2", "badcrc", "noise", "signs", "zeros", "tie", "nan", "inf", "ninf")
IDX = {n: k for k, n in enumerate(NAMES)}


@functools.lru_cache(maxsize=None)
def generator(seed):
    """The generator the restatement derives from the seed's H (any basis gives the same records)."""
    G, rank = O.generator(C.make_code(seed)["code"].H)
    assert rank == 83
    G.setflags(write=False)
    return G


def noisy(seed, sseed):
    rng = np.random.default_rng(1000 * sseed + 85)
    m = C.message91(rng)
    cw = C.encode(seed, m)
    return (2.83 * ((2.0 * cw - 1.0) + NOISE * rng.standard_normal(N))).astype(F32), m


TIE_SSEED = 6                               # under both codes this noise seed gives a tie (found by search; the inputs test proves it)


def tie_set(seed):
    """Two equal-distance winners that the flip-count rule separates: a codeword in noise with the metrics rounded to whole numbers, 2 (s + 0.9
    N(0, 1)), so that every distance is a small integer, exact in float32, and equal distances are common.  -> (llr, the 91 bits sent)."""
    rng = np.random.default_rng(5000 + TIE_SSEED)
    m = C.message91(rng)
    cw = C.encode(seed, m)
    return np.round(2.0 * ((2.0 * cw - 1.0) + 0.9 * rng.standard_normal(N))).astype(F32), m


@functools.lru_cache(maxsize=None)
def metric_sets(seed):
    """-> (llr float32[12, 174] in NAMES' order, [the 91 bits sent or None])."""
    rng = np.random.default_rng(seed + 5)
    sets = {}
    m = C.message91(rng)
    sets["clean"] = ((2.83 * (2.0 * C.encode(seed, m) - 1.0)).astype(F32), m)
    for name in ("h1", "h2", "o2"):
        sets[name] = noisy(seed, NOISY[seed][name])
    m = C.message91(rng, flip_crc=True)
    sets["badcrc"] = ((2.83 * (2.0 * C.encode(seed, m) - 1.0)).astype(F32), m)
    sets["noise"] = ((F32(2.83) * rng.standard_normal(N)).astype(F32), None)
    sets["signs"] = ((F32(3) * (2 * rng.integers(0, 2, N) - 1)).astype(F32), None)
    sets["zeros"] = (np.zeros(N, F32), None)
    sets["tie"] = tie_set(seed)
    for name, pos, val in (("nan", 100, np.nan), ("inf", 3, np.inf), ("ninf", 173, -np.inf)):
        llr = sets["h1"][0].copy()
        llr[pos] = val
        sets[name] = (llr, None)
    llr = np.stack([sets[n][0] for n in NAMES])
    llr.setflags(write=False)
    return llr, [sets[n][1] for n in NAMES]


@functools.lru_cache(maxsize=None)
def reference_records(seed, order):
    """The restatement's records of metric_sets(seed): computed once, shared by the tests."""
    rec = O.decode(generator(seed), metric_sets(seed)[0], order)
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def bp_records(seed):
    """Belief propagation (30 iterations) on the finite sets; the rest are not attempted."""
    llr = metric_sets(seed)[0]
    return R.decode(C.make_code(seed)["code"], np.nan_to_num(llr, nan=0.0, posinf=0.0, neginf=0.0), 30, np.isfinite(llr).all(axis=1))


# ---- the chain case: ldpc_cases.CHAIN's three 48 kHz FT8 channels, noise and messages, with some transmissions weakened ------------------------
# (dial offset, [(audio Hz of tone 0, start s, amplitude, message seed)]).  The amplitudes were searched on the CPU oracle's frames (a scale on
# ldpc_cases.CHAIN's, per transmission) for strongest candidates that belief propagation at 30 iterations does NOT bring to crc_ok and OSD at
# order 2 returns with crc_ok and the sent message; the others keep their amplitude and decode by belief propagation, so OSD must leave them
# alone.  CHAIN_RECOVERED names, per code, the transmissions (message seeds) of the first kind: tests/test_osd_cases_inputs.py proves them.
CHAIN_FS, CHAIN_BLK, CHAIN_N, CHAIN_SIGMA, CHAIN_SYNC = C.CHAIN_FS, C.CHAIN_BLK, C.CHAIN_N, C.CHAIN_SIGMA, C.CHAIN_SYNC
CHAIN = [(-15000, [(500.0, 0.52, 860.0, 301), (1250.0, 1.00, 1300.0, 302), (2062.5, 0.20, 770.0, 303)]),
         (2000, [(718.75, 0.60, 1200.0, 304), (1875.0, 1.40, 860.0, 305)]),
         (11000, [(1000.0, 0.32, 814.0, 306), (1562.5, 0.80, 1400.0, 307), (2500.0, 1.20, 740.0, 308)])]
CHAIN_MAX_ITER, CHAIN_MIN_NSYNC, CHAIN_ORDER, CHAIN_OSD_MIN_NSYNC = 30, 7, 2, 7
CHAIN_RECOVERED = {1741: (301, 303, 305, 306, 308), 9183: (303, 305, 308)}
CHAIN_BP = (302, 304, 307)                  # decoded by belief propagation under both codes: OSD does not attempt them
QUIET_RF, QUIET_SYNCMIN = 6000, 2.0         # a dial offset with noise alone: at syncmin 2.0 its list is empty while every transmission is still found


@functools.lru_cache(maxsize=None)
def chain_iq(seed):
    """The slot of IQ (complex64[CHAIN_N]) under the code of `seed`: ldpc_cases.chain_iq with CHAIN's amplitudes."""
    rng = np.random.default_rng(4242)
    iq = (rng.normal(0.0, CHAIN_SIGMA, CHAIN_N) + 1j * rng.normal(0.0, CHAIN_SIGMA, CHAIN_N)).astype(np.complex64)
    for rf, txs in CHAIN:
        for audio, t0, amp, mseed in txs:
            iq = iq + C.iq_of_tones(CHAIN_FS, CHAIN_N, rf, audio, t0, amp, C.tones_of(C.encode(seed, C.chain_message(mseed))))
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq
