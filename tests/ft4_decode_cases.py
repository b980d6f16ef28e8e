"""Test helper: FT4 transmissions that carry real codewords of the seed codes (tests/ldpc_cases.py), the recipes the FT4 decode tests share, and
expected(): the numpy restatement (tests/ldpc_ref.py) applied per metric set to cwslg_ft4_soft records with the two gates of
cwslg_enable_ft4_decode -> cwslg_ft4_msg records (60 bytes).  tests/test_ft4_decode_inputs.py vets the recipes on the CPU oracle's records; if a
property is missing there the recipes change, not the assertions."""
import functools

import numpy as np

import ft4_softbits_ref as S
import ldpc_cases as C
import ldpc_ref as R
from ft8_signal import ICOS4

F32 = np.float32
FS, BLK = 48000, 1024
N4 = int(7.5 * FS) // BLK * BLK             # one FT4 slot of IQ
MSG4_DTYPE = np.dtype([("set", R.MSG_DTYPE, 3)])
assert MSG4_DTYPE.itemsize == 60
SYNC = dict(syncmin=1.5, f_lo=200, f_hi=3000)
MAX_CAND = 100                              # the chain's list limit: above every recipe's list length, so the transmissions are in the list


def tones_of(cw):
    """103 channel tones of a 174-bit codeword: the inverse of ft4_softbits_ref.tone_bits (two bits per data symbol, MSB first, through graymap),
    Costas blocks at symbols 0, 33, 66, 99."""
    v = np.asarray(cw, int).reshape(87, 2) @ np.array([2, 1])
    t = np.zeros(S.NN, int)
    t[S.DATA_SYMBOLS] = S.GRAYMAP[v]
    for b, base in enumerate((0, 33, 66, 99)):
        t[base:base + 4] = ICOS4[b]
    return t


def iq_of_tones(n, rf_hz, audio_hz, t0_s, amp, tones):
    """Complex IQ of one FT4 transmission with the given tones (ft4_softbits_ref.ft4_iq_with_tones with the tones supplied, t0_s >= 0)."""
    ph = S._phase(np.asarray(tones), rf_hz + audio_hz, int(round(FS * 0.048)), FS)
    out = np.zeros(n, np.complex64)
    i0 = int(round(t0_s * FS))
    m = min(len(ph), n - i0)
    out[i0:i0 + m] = amp * np.exp(1j * ph[:m])
    return out


def message(mseed):
    return C.message91(np.random.default_rng(mseed))


# ---- recipes: name -> (noise sigma per component, noise seed, [(dial offset Hz, [(audio Hz of tone 0, start s, amplitude, message seed)])]) --------------
# One slot of IQ at 48 kHz holds every channel of a recipe.  The levels are chosen (tests/test_ft4_decode_inputs.py checks it) so that every
# transmission decodes with crc_ok in some set and at least one decode needs an iteration.  The search threshold SYNCMIN_FT4 is lowered from
# upstream's 1.2 so that the lists have a tail of candidates that are noise: they bring the records below nsync 8 and below nqual 20, candidates
# with two and three records, and lists longer than a small max_cand (a list that is cut keeps its FIRST candidates in frequency order, as
# getcandidates4 does, so the transmissions are looked for under MAX_CAND only).  A channel with no transmissions is noise only; at SYNCMIN_QUIET it has
# no candidate at all while the transmissions of the other channels are still found.
# "carriers" is a frame of another kind: three unmodulated carriers of very different levels over weak noise.  Their skirts raise candidates the
# refinement then finds nothing in (all three segments below 1.2): at HOLES_MAX_CAND the cut list holds candidates with 0, 1, 2 and 3 records.
SIGMA = 26000.0
SYNCMIN_FT4, SYNCMIN_QUIET = 1.0, 2.0
RECIPES = {
    # (noise seed None: the last N4 samples of ldpc_cases.chain_iq -- noise of the same level and the FT8 chain case's transmissions, which lie
    # outside these two passbands -- so that one stretch of IQ serves FT4 and FT8 channels side by side)
    "chain": (SIGMA, None, [(-9000, [(700.0, 0.50, 1900.0, 401), (1600.0, 0.90, 1300.0, 402), (2450.0, 0.30, 1500.0, 403)]),
                            (6000, [(1000.0, 0.70, 1700.0, 404), (2100.0, 0.40, 1400.0, 405)])]),
    "small": (SIGMA, 5252, [(9000, [(1300.0, 0.80, 1700.0, 412), (2200.0, 0.35, 1500.0, 413)]),
                            (-6000, [])]),
    "carriers": (1.0, 5454, [(-3000, [])]),
}
CARRIERS = {"carriers": [(-3000, 700.0, 3000.0), (-3000, 1500.0, 1000.0), (-3000, 2300.0, 300.0)]}      # name -> [(dial offset Hz, audio Hz, amplitude)]
HOLES_MAX_CAND = 17                         # 153 waves per channel: the list is cut and one of its candidates has no record
FT8_CHAIN = C.CHAIN[2]                      # the FT8 channel that runs beside the "chain" recipe: ldpc_cases' third chain channel (11 kHz)
assert C.CHAIN_FS == FS and C.CHAIN_N % BLK == 0 and (C.CHAIN_N - N4) % BLK == 0 and C.CHAIN_SIGMA == SIGMA


@functools.lru_cache(maxsize=None)
def recipe_iq(name, seed):
    """The slot of IQ (complex64[N4]) of a recipe under the code of `seed`; read-only."""
    sigma, nseed, chans = RECIPES[name]
    if nseed is None:
        iq = np.array(C.chain_iq(seed)[-N4:])
    else:
        rng = np.random.default_rng(nseed)
        iq = (rng.normal(0.0, sigma, N4) + 1j * rng.normal(0.0, sigma, N4)).astype(np.complex64)
    for rf, txs in chans:
        for audio, t0, amp, mseed in txs:
            iq = iq + iq_of_tones(N4, rf, audio, t0, amp, tones_of(C.encode(seed, message(mseed))))
    t = np.arange(N4) / FS
    for rf, audio, amp in CARRIERS.get(name, []):
        iq = iq + amp * np.exp(2j * np.pi * (rf + audio) * t)
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq


def soft_dict(llr, sigma, nsync, nqual):
    return dict(llr=np.asarray(llr, F32).reshape(-1, 3, 174), sigma=np.asarray(sigma, F32).reshape(-1, 3), nsync=np.asarray(nsync).reshape(-1),
                nqual=np.asarray(nqual).reshape(-1))


def expected(soft_records, code, max_iter, min_nsync, min_nqual):
    """soft_records: dict(llr [n, 3, 174], sigma [n, 3], nsync [n], nqual [n]) -> MSG4_DTYPE[n]: set s is ldpc_ref.decode of llr[:, s]; a record
    with nsync < min_nsync or nqual < min_nqual is not attempted in any set, otherwise set s is not attempted exactly when sigma[s] == 0."""
    r = soft_records
    n = len(r["nsync"])
    out = np.zeros(n, MSG4_DTYPE)
    gate = (r["nsync"] >= min_nsync) & (r["nqual"] >= min_nqual)
    for s in range(3):
        out["set"][:, s] = R.decode(code, r["llr"][:, s], max_iter, gate & (r["sigma"][:, s] != 0)) if n else np.zeros(0, R.MSG_DTYPE)
    return out


def best_set(rec):
    """The smallest s with crc_ok, -1 if none: int array [n]."""
    ok = rec["set"]["crc_ok"] != 0
    return np.where(ok.any(axis=1), ok.argmax(axis=1), -1)


def attempted(rec):
    return rec["set"]["iters"] >= 0


def find_message(rec, bits91):
    """Indices of the records whose best set carries exactly these 91 bits."""
    b = best_set(rec)
    return [q for q in range(len(rec)) if b[q] >= 0 and np.array_equal(R.unpack_bits(rec["set"]["bits"][q, b[q]]), bits91)]
