"""Test helper: the numpy restatement of the FT4 signal reports (include/cwsl_gpu.h, "FT4 signal reports") -- the 103 tones of a word under the
systematic re-encoder of tests/decode_reports_ref.py, and per decode nsync / nsymerr / xsig / xnoise / snr_db on the symbol spectra
ft4_softbits_ref.symbol_spectra makes of the baseband oracle.ft4_downsample gives at the record's f1_hz -- float32 throughout, the two 103-term
sums written out as the tree the header states.  PARITY UNPINNED like the rest of the sync stage."""
import numpy as np

import decode_reports_ref as RR
import ft4_softbits_ref as S4

F32 = np.float32
NN, NDATA = S4.NN, 87
ICOS4 = (0, 1, 3, 2, 1, 0, 2, 3, 2, 3, 1, 0, 3, 2, 0, 1)                # blocks 0132 1023 2310 3201 at symbols 0, 33, 66, 99
GRAYMAP = (0, 1, 3, 2)
COSTAS = tuple(33 * b + s for b in range(4) for s in range(4))
DATA = tuple(range(4, 33)) + tuple(range(37, 66)) + tuple(range(70, 99))  # data symbol d sits at DATA[d]
FLT_MAX = np.finfo(F32).max
REPORT_DTYPE = RR.REPORT_DTYPE
FLOOR_DB, OFFSET_DB = F32(-21.0), 20.8
assert tuple(S4.COSTAS_SYMBOLS) == COSTAS and tuple(S4.DATA_SYMBOLS) == DATA and tuple(S4.GRAYMAP) == GRAYMAP

encoder, codeword, word_bits, log10_fixed = RR.encoder, RR.codeword, RR.word_bits, RR.log10_fixed


def tones_of(cw):
    """103 tones of a 174-bit codeword (no rvec): the Costas blocks; data symbol d at DATA[d], tone graymap[2 cw[2d] + cw[2d+1]]."""
    t = np.zeros(NN, np.uint8)
    t[list(COSTAS)] = ICOS4
    for d in range(NDATA):
        t[DATA[d]] = GRAYMAP[2 * int(cw[2 * d]) + int(cw[2 * d + 1])]
    return t


def tones(G, bits12):
    return tones_of(codeword(G, bits12))


def powers(zr, zi):
    """P[n][q] = fmaf(re, re, im * im) of cs float32[103, 4]"""
    zr, zi = np.asarray(zr, F32), np.asarray(zi, F32)
    assert zr.shape == zi.shape == (NN, 4)
    return S4.fmaf(zr, zr, zi * zi)


def tree103(terms):
    """Lane l holds term l, plus term l + 64 for l < 39, added in that order; then a[l] = a[l] + a[l + h], h = 32 .. 1; a[0]."""
    t = np.asarray(terms, F32)
    assert t.shape == (NN,)
    a = t[:64].copy()
    a[:39] = a[:39] + t[64:103]
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
    db = F32(10.0 * log10_fixed(float(x)) - OFFSET_DB)
    return max(db, FLOOR_DB)


def _first_max(row):
    """The first maximum as the comparisons `v > vm` find it (a NaN never wins)."""
    km, vm = 0, row[0]
    for k in range(1, 4):
        if row[k] > vm:
            km, vm = k, row[k]
    return km


def report_of_spectra(zr, zi, t):
    """One decode from its cs[103][4] (re, im) and tones t[103]: a REPORT_DTYPE scalar."""
    P = powers(zr, zi)
    with np.errstate(invalid="ignore"):
        mag = np.sqrt(P, dtype=F32)
    first = np.argmax(mag, axis=1) if not np.isnan(mag).any() else np.array([_first_max(row) for row in mag])
    t = np.asarray(t, np.int64)
    hit = first == t
    out = np.zeros((), REPORT_DTYPE)
    out["nsync"] = int(hit[list(COSTAS)].sum())
    out["nsymerr"] = int((~hit[list(DATA)]).sum())
    with np.errstate(all="ignore"):
        out["xsig"] = tree103(P[np.arange(NN), t])
        out["xnoise"] = tree103(P[np.arange(NN), (t + 2) & 3])
    out["snr_db"] = snr_db(out["xsig"], out["xnoise"])
    return out


def report(cb, ibest, t):
    """One decode: cb complex64[4032] the baseband at the record's f1_hz, ibest its start, t the tones."""
    zr, zi = S4.symbol_spectra(np.asarray(cb, np.complex64).reshape(1, -1), [int(ibest)])
    return report_of_spectra(zr[0], zi[0], t)


def baseband(oracle, cx, f1_hz):
    return oracle.ft4_downsample(cx, F32(f1_hz))[0]


def reports(oracle, G, spectra, records, decodes):
    """The reports of `decodes` (records with ch_id, entry, bits): spectra[ch_id] complex64[36289] the channel's frame spectrum, records[ch_id]
    its sync records (f1_hz, ibest) in cwslg_fetch_ft4_sync's order, G the encoder in force.  -> REPORT_DTYPE[len(decodes)]."""
    out = np.zeros(len(decodes), REPORT_DTYPE)
    cache = {}
    for p, d in enumerate(decodes):
        ch, q = int(d["ch_id"]), int(d["entry"])
        if (ch, q) not in cache:
            r = records[ch][q]
            cb = baseband(oracle, spectra[ch], r["f1_hz"])
            cache[ch, q] = S4.symbol_spectra(np.asarray(cb, np.complex64).reshape(1, -1), [int(r["ibest"])])
        zr, zi = cache[ch, q]
        out[p] = report_of_spectra(zr[0], zi[0], tones(G, d["bits"]))
    return out
