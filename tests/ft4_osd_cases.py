"""Test helper: the FT4 frames the FT4 OSD tests share, and expected(): the numpy restatement (tests/osd_ref.py) applied per metric set to
cwslg_ft4_soft and cwslg_ft4_msg records with the record-level gate of cwslg_enable_ft4_osd -> cwslg_ft4_osd records (72 bytes).
tests/test_ft4_osd_inputs.py vets the recipes on the CPU oracle's records; if a property is missing there the recipes change, not the
assertions."""
import functools

import numpy as np

import ft4_decode_cases as D
import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O

F32 = np.float32
FS, BLK, N4 = D.FS, D.BLK, D.N4
SEEDS = C.SEEDS
OSD4_DTYPE = np.dtype([("set", O.OSD_DTYPE, 3)])
assert OSD4_DTYPE.itemsize == 72
SYNC, MAX_CAND, SYNCMIN_FT4, SYNCMIN_QUIET, HOLES_MAX_CAND = D.SYNC, D.MAX_CAND, D.SYNCMIN_FT4, D.SYNCMIN_QUIET, D.HOLES_MAX_CAND
MAX_ITER, MIN_NSYNC, MIN_NQUAL, ORDER = 30, 8, 20, 2        # the decode's and the OSD's gates are the same pair in every chain test
generator = OC.generator

# ---- recipes ------------------------------------------------------------------------------------------------------------------------------------
# ft4_decode_cases.RECIPES["small"] (dial 9000 with two transmissions, dial -6000 with noise alone, noise seed 5252, sigma 26000) with the two
# amplitudes scaled, per test code, by factors searched on the CPU oracle's records: in each frame one transmission decodes by belief
# propagation (so its record is not attempted by OSD), the other is left without crc_ok in all three sets and comes back from OSD at order 2
# with the 91 bits sent, and some record of the list has BP crc_ok in some but not all sets -- where the record-level gate differs from a
# per-set one.  "weak" is a second frame per code in which OSD finds its word with the other flip count, so that how is 1 once and 2 once per
# code.  name -> {code seed -> (factor of message 412, factor of message 413)}; RECOVERED / BP / HOW name what the inputs test proves.
BASE = D.RECIPES["small"]
RECIPES = {"main": {1741: (0.72, 0.72), 9183: (0.72, 0.80)},
           "weak": {1741: (0.64, 0.64), 9183: (0.60, 0.60)}}
RECOVERED = {"main": {1741: (413,), 9183: (413,)}, "weak": {1741: (412,), 9183: (412,)}}    # message seeds OSD returns where BP failed in all three sets
BP = {"main": {1741: (412,), 9183: (412,)}, "weak": {1741: (), 9183: ()}}                    # message seeds BP decodes: their records are not attempted
HOW = {"main": {1741: 2, 9183: 1}, "weak": {1741: 1, 9183: 2}}                              # flips of the first RECOVERED word
PARTIAL = {"main": {1741: True, 9183: True}}                                                 # a record with BP crc_ok in some but not all sets
RF_TX, RF_NOISE = BASE[2][0][0], BASE[2][1][0]


def transmissions(name, seed):
    """[(audio Hz of tone 0, start s, amplitude, message seed)] of the recipe's one occupied channel."""
    f = dict(zip((412, 413), RECIPES[name][seed]))
    return [(audio, t0, amp * f[mseed], mseed) for audio, t0, amp, mseed in BASE[2][0][1]]


@functools.lru_cache(maxsize=None)
def recipe_iq(name, seed):
    """The slot of IQ (complex64[N4]) of a recipe under the code of `seed`; read-only.  "carriers" and "small" are ft4_decode_cases' frames."""
    if name in D.RECIPES:
        return D.recipe_iq(name, seed)
    sigma, nseed, _ = BASE
    rng = np.random.default_rng(nseed)
    iq = (rng.normal(0.0, sigma, N4) + 1j * rng.normal(0.0, sigma, N4)).astype(np.complex64)
    for audio, t0, amp, mseed in transmissions(name, seed):
        iq = iq + D.iq_of_tones(N4, RF_TX, audio, t0, amp, D.tones_of(C.encode(seed, D.message(mseed))))
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq


def gate(soft, msg, min_nsync, min_nqual):
    """bool[n, 3]: set s of record q is attempted iff its decode record was attempted, NO set of the record has BP crc_ok, and nsync and nqual
    pass."""
    rec_ok = ~(msg["set"]["crc_ok"] != 0).any(axis=1) & (np.asarray(soft["nsync"]) >= min_nsync) & (np.asarray(soft["nqual"]) >= min_nqual)
    return (msg["set"]["iters"] >= 0) & rec_ok[:, None]


def expected(soft, msg, G, order, min_nsync, min_nqual):
    """soft: dict(llr [n, 3, 174], sigma, nsync [n], nqual [n]); msg: cwslg_ft4_msg records [n] -> OSD4_DTYPE[n]: set s is osd_ref.decode of
    llr[:, s] under gate()."""
    n = len(msg)
    out = np.zeros(n, OSD4_DTYPE)
    if n == 0:
        return out
    att = gate(soft, msg, min_nsync, min_nqual)
    for s in range(3):
        out["set"][:, s] = O.decode(G, soft["llr"][:, s], order, att[:, s])
    return out


def per_set_gate(soft, msg, min_nsync, min_nqual):
    """The gate this stage does NOT have (each set on its own crc_ok): the inputs test shows a record on which the two differ."""
    ok = (np.asarray(soft["nsync"]) >= min_nsync) & (np.asarray(soft["nqual"]) >= min_nqual)
    return (msg["set"]["iters"] >= 0) & (msg["set"]["crc_ok"] == 0) & ok[:, None]


def best_word(msg, osd):
    """-> (s int[n], by_osd bool[n]): the smallest s with BP crc_ok; otherwise the smallest s with OSD crc_ok, by_osd set; otherwise -1."""
    bp = msg["set"]["crc_ok"] != 0
    ok = osd["set"]["crc_ok"] != 0
    has_bp = bp.any(axis=1)
    by_osd = ~has_bp & ok.any(axis=1)
    return np.where(has_bp, bp.argmax(axis=1), np.where(by_osd, ok.argmax(axis=1), -1)), by_osd


def attempted(osd):
    return osd["set"]["how"] != 0xff


def word_bits(msg, osd, q):
    """The 91 bits of record q's best word, None if it has none; and whether OSD found it."""
    s, by = best_word(msg[q:q + 1], osd[q:q + 1])
    if s[0] < 0:
        return None, False
    src = osd if by[0] else msg
    return R.unpack_bits(src["set"]["bits"][q, s[0]]), bool(by[0])


def find_word(msg, osd, bits91):
    """[(record index, by_osd)] of the records whose best word carries exactly these 91 bits."""
    out = []
    for q in range(len(msg)):
        b, by = word_bits(msg, osd, q)
        if b is not None and np.array_equal(b, bits91):
            out.append((q, by))
    return out


@functools.lru_cache(maxsize=None)
def rank_deficient_table():
    """A parity-check table cwslg_set_ldpc_code accepts (every position exactly three times, none twice in a row, rows of 6 or 7 entries) whose H
    has rank 82: rows 0, 1 and 2 share their 18 entries pairwise (columns 0..8 have two of their three ones among them), so the three rows sum
    to zero.  Belief propagation runs on it; OSD cannot.  -> nm uint8[83, 7]."""
    M = 83
    rows = [[] for _ in range(M)]
    pairs = [(0, 1)] * 3 + [(0, 2)] * 3 + [(1, 2)] * 3
    for col, (a, b) in enumerate(pairs):
        for m in (a, b, 3 + col):
            rows[m].append(col + 1)
    cap = np.array([6] * 3 + [7] * 24 + [6] * 56) - np.array([len(r) for r in rows])      # rows 0..2 are full; 24 rows of 7, 56 of 6 entries remain
    for col in range(9, O.N):
        for m in np.argsort(-cap, kind="stable")[:3]:
            rows[m].append(col + 1)
            cap[m] -= 1
    assert not cap.any()
    nm = np.zeros((M, 7), np.uint8)
    for m, r in enumerate(rows):
        nm[m, :len(r)] = r
    nm.setflags(write=False)
    return nm
