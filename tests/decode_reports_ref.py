"""Test helper: the numpy restatement of cwslg_decode_report (include/cwsl_gpu.h, "FT8 signal reports") -- the systematic re-encoder derived from
a parity-check table, the 79 tones of a word, and per decode nsync / nsymerr / xsig / xnoise / snr_db on a symbol-spectra plane, float32 throughout
with the two 79-term sums written out as the tree the header states.  Nothing here comes from the library or from ldpc_cases: the table is the
only input.  PARITY UNPINNED like the rest of the sync stage."""
import numpy as np

F32 = np.float32
N, K, M = 174, 91, 83
NSYM, NHSYM, NH1 = 79, 372, 1920
ICOS7 = (3, 1, 4, 0, 6, 5, 2)
GRAYMAP = (0, 1, 3, 2, 5, 6, 4, 7)
COSTAS = tuple(base + r for base in (0, 36, 72) for r in range(7))
DATA = tuple(range(7, 36)) + tuple(range(43, 72))                       # data symbol d sits at DATA[d]
FLT_MAX = np.finfo(F32).max
REPORT_DTYPE = np.dtype([("snr_db", F32), ("xsig", F32), ("xnoise", F32), ("nsync", np.int16), ("nsymerr", np.int16)])
assert REPORT_DTYPE.itemsize == 16


# ---- the re-encoder --------------------------------------------------------------------------------------------------------------------------------
def parity_matrix(nm):
    """H uint8[83, 174] of a table nm[83][7] (1-based positions, 0 = no entry)."""
    H = np.zeros((M, N), np.uint8)
    for m, row in enumerate(np.asarray(nm).reshape(M, 7)):
        for v in row:
            if v:
                H[m, int(v) - 1] ^= 1
    return H


def encoder(nm):
    """The systematic encoder of the code: G uint8[91, 174], row k the codeword of the unit message e_k -- or None when columns 91..173 of H are
    singular.  H is reduced taking pivots in columns 91..173 only."""
    A = parity_matrix(nm)
    for r in range(M):
        c = K + r
        rows = [p for p in range(r, M) if A[p, c]]
        if not rows:
            return None
        A[[r, rows[0]]] = A[[rows[0], r]]
        for i in range(M):
            if i != r and A[i, c]:
                A[i] ^= A[r]
    G = np.zeros((K, N), np.uint8)
    G[:, :K] = np.eye(K, dtype=np.uint8)
    G[:, K:] = A[:, :K].T                                               # parity bit 91 + r of e_k: the entry of reduced row r in column k
    return G


def word_bits(bits12):
    """The 91 message bits of bits[12], MSB first."""
    return np.unpackbits(np.frombuffer(bytes(bytearray(np.asarray(bits12, np.uint8).tolist())), np.uint8))[:K]


def codeword(G, bits12):
    return (word_bits(bits12).astype(np.int64) @ G.astype(np.int64) % 2).astype(np.uint8)


def tones_of(cw):
    """79 tones of a 174-bit codeword: Costas at 0..6, 36..42, 72..78; data symbol d at DATA[d], tone graymap[4 cw[3d] + 2 cw[3d+1] + cw[3d+2]]."""
    t = np.zeros(NSYM, np.uint8)
    for base in (0, 36, 72):
        t[base:base + 7] = ICOS7
    for d in range(58):
        t[DATA[d]] = GRAYMAP[4 * int(cw[3 * d]) + 2 * int(cw[3 * d + 1]) + int(cw[3 * d + 2])]
    return t


def tones(G, bits12):
    return tones_of(codeword(G, bits12))


# ---- the report --------------------------------------------------------------------------------------------------------------------------------------
def log10_fixed(x):
    """The library's fixed double-precision log10 (oracle/sync_oracle.c: orc_log10_fixed), operation for operation in IEEE doubles."""
    x = float(x)
    if not x > 0.0:
        return -1.0e300
    assert x < float("inf")
    e, m = 0, x
    while m >= 1.4142135623730951:
        m = m * 0.5
        e += 1
    while m < 0.7071067811865476:
        m = m * 2.0
        e -= 1
    t = (m - 1.0) / (m + 1.0)
    t2 = t * t
    s = 0.0
    for k in range(21, 0, -2):
        s = s * t2 + 1.0 / float(k)
    ln_m = 2.0 * t * s
    return (float(e) * 0.6931471805599453 + ln_m) * 0.4342944819032518


def plane_powers(plane, i, j):
    """P float32[79, 8]: P[n][k] = S(i + 2k, m), m = j + 12 + 4n; +0 where m < 1, m > 372, the bin is above 1920 or beyond the row (or below 0)."""
    sp = np.asarray(plane)
    assert sp.dtype == F32 and sp.ndim == 2 and sp.shape[0] == NHSYM
    P = np.zeros((NSYM, 8), F32)
    for n in range(NSYM):
        m = int(j) + 12 + 4 * n
        if m < 1 or m > NHSYM:
            continue
        for k in range(8):
            b = int(i) + 2 * k
            if 0 <= b <= NH1 and b < sp.shape[1]:
                P[n, k] = sp[m - 1, b]
    return P


def tree79(terms):
    """Lane l holds term l, plus term l + 64 where that is below 79, added in that order; then a[l] = a[l] + a[l + h], h = 32 .. 1; a[0]."""
    t = np.asarray(terms, F32)
    assert t.shape == (NSYM,)
    a = t[:64].copy()
    a[:15] = a[:15] + t[64:79]
    h = 32
    while h >= 1:
        a = a[:h] + a[h:2 * h]
        h //= 2
    assert a.dtype == F32 and a.shape == (1,)
    return a[0]


def snr_db(xsig, xnoise):
    xsig, xnoise = F32(xsig), F32(xnoise)
    with np.errstate(all="ignore"):
        r = xsig / xnoise - F32(1.0) if xnoise > 0 else F32(0.0)
    x = r if r > F32(0.1) else F32(0.001)
    x = min(x, FLT_MAX)
    db = F32(10.0 * log10_fixed(float(x)) - 27.0)
    return max(db, F32(-24.0))


def report(plane, i, j, t):
    """One decode: (snr_db, xsig, xnoise, nsync, nsymerr) as a REPORT_DTYPE scalar."""
    P = plane_powers(plane, i, j)
    with np.errstate(invalid="ignore"):
        s8 = np.sqrt(P, dtype=F32)
    first = np.argmax(s8, axis=1) if not np.isnan(s8).any() else np.array([_first_max(row) for row in s8])
    t = np.asarray(t, np.int64)
    hit = first == t
    out = np.zeros((), REPORT_DTYPE)
    out["nsync"] = int(hit[list(COSTAS)].sum())
    out["nsymerr"] = int((~hit[list(DATA)]).sum())
    with np.errstate(all="ignore"):
        out["xsig"] = tree79(P[np.arange(NSYM), t])
        out["xnoise"] = tree79(P[np.arange(NSYM), (t + 4) % 7])
    out["snr_db"] = snr_db(out["xsig"], out["xnoise"])
    return out


def _first_max(row):
    """The first maximum as the comparisons `v > vm` find it (a NaN never wins)."""
    km, vm = 0, row[0]
    for k in range(1, 8):
        if row[k] > vm:
            km, vm = k, row[k]
    return km


def reports(G, planes, lists, decodes):
    """The reports of `decodes` (records with ch_id, entry, bits): planes[ch_id] float32[372, pitch], lists[ch_id] the candidates
    (freq_bin, time_step, ...) of the channel, G the encoder in force.  -> REPORT_DTYPE[len(decodes)]."""
    out = np.zeros(len(decodes), REPORT_DTYPE)
    for p, d in enumerate(decodes):
        ch, c = int(d["ch_id"]), lists[int(d["ch_id"])][int(d["entry"])]
        out[p] = report(planes[ch], int(c[0]), int(c[1]), tones(G, d["bits"]))
    return out
