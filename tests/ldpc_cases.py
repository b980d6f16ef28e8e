"""Test helper: (174, 91) codes of the shape cwslg_set_ldpc_code takes, made from a seed -- the upstream table is not in this repository and no test
needs it: nothing in the decoder depends on which table it is -- with a systematic encoder, the CRC-14 message helper, FT8 tones / IQ of a codeword,
and the metric sets the decode tests share (tests/test_ldpc_cases_inputs.py checks with the restatement alone that they reach every exit)."""
import functools

import numpy as np

import ldpc_ref as R
from ft8_signal import ICOS7

F32 = np.float32
N, K, M = R.N, R.K, R.M
SEEDS = (1741, 9183)                        # two seeds, two different codes
GRAYMAP = np.array([0, 1, 3, 2, 5, 6, 4, 7])


def _gf2_rank_pivots(H):
    """Row-reduce a copy of H over GF(2) taking pivots from the LAST column backwards.  -> (rank, pivot columns)."""
    A = H.copy() % 2
    piv, r = [], 0
    for c in range(A.shape[1] - 1, -1, -1):
        rows = np.nonzero(A[r:, c])[0]
        if rows.size == 0:
            continue
        A[[r, r + rows[0]]] = A[[r + rows[0], r]]
        for i in np.nonzero(A[:, c])[0]:
            if i != r:
                A[i] ^= A[r]
        piv.append(c)
        r += 1
        if r == A.shape[0]:
            break
    return r, piv


def _gf2_inv(B):
    n = B.shape[0]
    A = np.concatenate([B % 2, np.eye(n, dtype=np.uint8)], axis=1)
    for c in range(n):
        rows = np.nonzero(A[c:, c])[0]
        assert rows.size, "singular"
        A[[c, c + rows[0]]] = A[[c + rows[0], c]]
        for i in np.nonzero(A[:, c])[0]:
            if i != c:
                A[i] ^= A[c]
    return A[:, n:]


def _try_table(rng):
    """One attempt: column weight 3, 59 rows of weight 6 and 24 of weight 7, no two rows sharing two columns (no 4-cycles).  -> H or None."""
    cap = np.full(M, 6)
    cap[rng.choice(M, 24, replace=False)] = 7
    used = np.zeros((M, M), bool)                                       # row pairs that already share a column
    H = np.zeros((M, N), np.uint8)
    for n in range(N):
        rows = []
        for m in np.argsort(-(cap + rng.random(M))):                    # fullest remaining capacity first, ties at random
            if cap[m] > 0 and not any(used[m, r] for r in rows):
                rows.append(int(m))
                if len(rows) == 3:
                    break
        if len(rows) < 3:
            return None
        for a in rows:
            cap[a] -= 1
            H[a, n] = 1
            for b in rows:
                if a != b:
                    used[a, b] = True
    return H if not cap.any() else None


@functools.lru_cache(maxsize=None)
def make_code(seed):
    """-> dict(nm uint8[83, 7], code ldpc_ref.Code, P uint8[83, 91]: parity bits = P m over GF(2), codeword = message ++ parity)."""
    rng = np.random.default_rng(seed)
    while True:
        H = _try_table(rng)
        if H is None:
            continue
        H = H[:, rng.permutation(N)]
        rank, piv = _gf2_rank_pivots(H)
        if rank == M:
            break
    # columns: the 83 pivot columns last (they are invertible), the others first, both in their order of appearance
    rest = [c for c in range(N) if c not in set(piv)]
    H = H[:, rest + sorted(piv)]
    assert (H.sum(axis=0) == 3).all() and sorted(H.sum(axis=1)) == [6] * 59 + [7] * 24
    assert ((H.astype(int) @ H.T.astype(int))[~np.eye(M, dtype=bool)] <= 1).all(), "4-cycle"
    assert _gf2_rank_pivots(H)[0] == M
    P = (_gf2_inv(H[:, K:]).astype(int) @ H[:, :K].astype(int)) % 2     # H [m; p] = 0  ->  p = B^-1 A m
    nm = np.zeros((M, 7), np.uint8)
    for m in range(M):
        cols = rng.permutation(np.nonzero(H[m])[0]) + 1                 # a row's entries in no particular order: the order is part of the contract
        nm[m, :len(cols)] = cols
    code = R.Code(nm)
    assert np.array_equal(code.H, H)
    return dict(nm=nm, code=code, P=P.astype(np.uint8))


def encode(seed, bits91):
    c = make_code(seed)
    m = np.asarray(bits91, np.uint8)
    cw = np.concatenate([m, (c["P"].astype(int) @ m.astype(int)) % 2]).astype(np.uint8)
    assert not ((c["code"].H.astype(int) @ cw) % 2).any()
    return cw


def message91(rng, flip_crc=False):
    """77 random bits + their CRC-14, MSB first (flip_crc: the CRC field's last bit inverted -- a codeword's worth of bits whose CRC is wrong)."""
    b = rng.integers(0, 2, 77).astype(np.uint8)
    crc = R.crc14(b)
    out = np.concatenate([b, [(crc >> (13 - i)) & 1 for i in range(14)]]).astype(np.uint8)
    if flip_crc:
        out[90] ^= 1
    return out


def tones_of(cw):
    """79 channel tones of a 174-bit codeword: three bits per data symbol, MSB first, through graymap; Costas blocks at 0, 36, 72."""
    v = np.asarray(cw, int).reshape(58, 3) @ np.array([4, 2, 1])
    data = GRAYMAP[v]
    return np.concatenate([ICOS7, data[:29], ICOS7, data[29:], ICOS7])


def iq_of_tones(fs, n, rf_hz, audio_hz, t0_s, amp, tones):
    """Complex baseband of one FT8 transmission with the given tones (tests/ft8_signal.py:ft8_iq with the tones supplied)."""
    sps = int(round(fs * 0.16))
    f = rf_hz + audio_hz + 6.25 * np.repeat(np.asarray(tones), sps)
    ph = 2 * np.pi * np.cumsum(f) / fs
    out = np.zeros(n, np.complex64)
    i0 = int(round(t0_s * fs))
    m = min(len(ph), n - i0)
    out[i0:i0 + m] = (amp * np.exp(1j * ph))[:m]
    return out


# ---- the metric sets of the stand-alone decode tests -------------------------------------------------------------------------------------------
# (kind, seed of the set, noise level): llr = 2.83 (s + noise x N(0, 1)) with s = +-1 the codeword ("cw"; "badcrc": a codeword whose CRC field is
# wrong), 2.83 noise x N(0, 1) alone ("noise"), +-3 at random ("signs"), all +0 ("zeros").  The noise levels are the case list's: 0 (clean), 0.45,
# 0.62 and 0.8 for codewords.  What each set is FOR is what tests/test_ldpc_cases_inputs.py asserts, under both codes.
NOISE_LEVELS = (0.45, 0.62, 0.8)
SETS = [("cw", 11, 0.0), ("badcrc", 12, 0.0), ("cw", 13, 0.45), ("cw", 14, 0.62), ("noise", 15, 1.0), ("signs", 16, 0.0), ("cw", 17, 0.8),
        ("cw", 28, 0.8), ("zeros", 19, 0.0)]
MAX_ITERS = (5, 30)
BATCHES = (0, 1, 3, 4, 5, 9)                # empty, one wave, a partial and a full workgroup, the step into the next, three workgroups


def metric_set(seed, kind, sseed, noise):
    """-> (llr float32[174], the 91 bits sent or None)."""
    rng = np.random.default_rng(1000 * sseed + 7)
    if kind == "zeros":
        return np.zeros(N, F32), None
    if kind == "noise":
        return (F32(2.83) * rng.standard_normal(N)).astype(F32), None
    if kind == "signs":
        return (F32(3) * (2 * rng.integers(0, 2, N) - 1)).astype(F32), None
    m = message91(rng, flip_crc=(kind == "badcrc"))
    cw = encode(seed, m)
    s = 2.0 * cw - 1.0
    return (2.83 * (s + noise * rng.standard_normal(N))).astype(F32), m


@functools.lru_cache(maxsize=None)
def metric_sets(seed):
    """-> (llr float32[9, 174], [bits sent or None]) of SETS under the code of `seed`."""
    sets = [metric_set(seed, *s) for s in SETS]
    return np.stack([s[0] for s in sets]), [s[1] for s in sets]


@functools.lru_cache(maxsize=None)
def reference_records(seed, max_iter):
    """The restatement's records of metric_sets(seed): computed once, shared by the tests."""
    rec = R.decode(make_code(seed)["code"], metric_sets(seed)[0], max_iter)
    rec.setflags(write=False)
    return rec


BAD_TABLES = ("position_175", "zero_inside", "weight_5", "twice_in_row", "four_times")


def bad_table(seed, kind):
    """A copy of the seed's table with one defect of the named kind."""
    nm = make_code(seed)["nm"].copy()
    w7 = int(np.nonzero(nm[:, 6] > 0)[0][0])
    w6 = int(np.nonzero(nm[:, 6] == 0)[0][0])
    if kind == "position_175":
        nm[3, 2] = 175
    elif kind == "zero_inside":                                          # a zero that is not the last entry
        nm[w7, 2], nm[w7, 6] = nm[w7, 6], 0
        nm[w7, 2], nm[w7, 3] = 0, nm[w7, 2]
    elif kind == "weight_5":                                             # a row of weight 5: its second zero cannot be last
        nm[w6, 5] = 0
    elif kind == "twice_in_row":
        nm[5, 1] = nm[5, 0]
    elif kind == "four_times":                                           # every row still well-formed, but one position four times and another twice
        other = next(int(v) for v in nm[1] if v and v not in nm[0])
        nm[0, 0] = other
    else:
        raise KeyError(kind)
    return nm


# ---- the chain case: three FT8 channels whose transmissions carry real codewords ----------------------------------------------------------------
# (dial offset, [(audio Hz of tone 0, start s, amplitude, message seed)]) at 48 kHz in Gaussian noise of CHAIN_SIGMA per component: the levels are
# chosen (tests/test_ldpc_cases_inputs.py checks it on the CPU oracle's frames) so that every transmission's strongest candidate decodes with
# crc_ok but not before the first iteration.  Tones sit on the search grid (3.125 Hz, 40 ms): the decode works on the plane's own grid.
CHAIN_FS, CHAIN_BLK = 48000, 2048
CHAIN_N = 720000 // CHAIN_BLK * CHAIN_BLK
CHAIN_SIGMA = 26000.0
CHAIN = [(-15000, [(500.0, 0.52, 1000.0, 301), (1250.0, 1.00, 1300.0, 302), (2062.5, 0.20, 1100.0, 303)]),
         (2000, [(718.75, 0.60, 1200.0, 304), (1875.0, 1.40, 1000.0, 305)]),
         (11000, [(1000.0, 0.32, 1100.0, 306), (1562.5, 0.80, 1400.0, 307), (2500.0, 1.20, 1000.0, 308)])]
CHAIN_SYNC = dict(syncmin=1.5, f_lo=200, f_hi=3000)


def chain_message(mseed):
    return message91(np.random.default_rng(mseed))


@functools.lru_cache(maxsize=None)
def chain_iq(seed):
    """The slot of IQ (complex64[CHAIN_N]) under the code of `seed`."""
    rng = np.random.default_rng(4242)
    iq = (rng.normal(0.0, CHAIN_SIGMA, CHAIN_N) + 1j * rng.normal(0.0, CHAIN_SIGMA, CHAIN_N)).astype(np.complex64)
    for rf, txs in CHAIN:
        for audio, t0, amp, mseed in txs:
            iq = iq + iq_of_tones(CHAIN_FS, CHAIN_N, rf, audio, t0, amp, tones_of(encode(seed, chain_message(mseed))))
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq
