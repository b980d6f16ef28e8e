"""numpy restatement of the FT4 subtractor (include/cwsl_gpu.h, "FT4 signal subtraction"): the contract's executable form.  Every float
operation below is one un-fused float32 operation in the order written; the integer phase is uint32 arithmetic modulo 2^32.  No cosine call: the
waveform comes from the committed tables (cwsl_digi_amd/csrc/modules/ft4sub_tables.inc, parsed here), so the device can agree on bits."""
import os
import re

import numpy as np

F32 = np.float32
U32 = np.uint32
HERE = os.path.dirname(os.path.abspath(__file__))
TABLES_INC = os.path.join(HERE, "..", "cwsl_digi_amd", "csrc", "modules", "ft4sub_tables.inc")

N = 72576                   # samples of a frame (the decoder's: F4C_NMAX)
NSPS = 576                  # samples of a symbol
NSYM = 103
NW = NSYM * NSPS            # samples of a signal, 59328
BLK = 18                    # samples of a block
BPS = NSPS // BLK           # 32 blocks per symbol
NBLK = NSYM * BPS           # 3296
NROWS = (NBLK + 255) // 256  # 13 rows of 256 blocks in the figures' tree
TAU_MAX, TAU_STEP = 54, 2   # time grid: -54, -52 .. +54 samples (55 offsets of 1/6 ms)
NTAU = 2 * TAU_MAX // TAU_STEP + 1
DINC, KF = 27962, 26        # frequency grid: k * DINC * 12000 / 2^32 Hz, k = -26..26 (steps of 0.078124 Hz, +-2.0312 Hz)
NK = 2 * KF + 1
HW = 48                     # half width of the track's window, in blocks
CAND_OFFSET = 0             # a record's dt_s names the transmission's first sample itself
TIME_STEP_S = TAU_STEP / 12000.0
FREQ_STEP_HZ = DINC * 12000.0 / 4294967296.0
R36 = F32(1.0) / F32(36.0)

SUB_DTYPE = np.dtype([("f_hz", F32), ("dt_s", F32), ("p_removed", F32), ("p_before", F32), ("p_after", F32), ("n_inside", np.int32),
                      ("df_steps", np.int16), ("dt_steps", np.int16)])
assert SUB_DTYPE.itemsize == 28


def parse_tables(path=TABLES_INC):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"FT4SUB_TABLE (float|unsigned) (\w+)\[(\d+)\] = \{([^}]*)\};", text):
        kind, name, count, body = m.group(1), m.group(2), int(m.group(3)), m.group(4)
        toks = [t for t in body.replace("\n", " ").split(",") if t.strip()]
        if kind == "float":
            arr = np.array([float.fromhex(t.strip().rstrip("f")) for t in toks], np.float64).astype(F32)
        else:
            arr = np.array([int(t.strip(), 16) for t in toks], np.uint64).astype(U32)
        assert arr.size == count, name
        out[name] = arr
    return out


_T = parse_tables()
CP = _T["FT4SUB_CP"].reshape(3, NSPS)
CPT = _T["FT4SUB_CPT"]
COSQ = _T["FT4SUB_COSQ"]
WIN = _T["FT4SUB_WIN"]


def _cos_of(idx):
    """cos of 2 pi idx / 4096 from the quarter table: C[r], -C[1024 - r], -C[r], C[1024 - r] in the four quarters (r = idx mod 1024)"""
    q, r = (idx >> 10) & 3, idx & 1023
    v = np.where((q & 1) == 0, COSQ[r], COSQ[1024 - r])
    return np.where((q == 1) | (q == 2), -v, v).astype(F32)


def cos_sin(phase):
    """(cos, sin) float32 of a uint32 phase (any integer array, taken modulo 2^32): the table index is the top 12 bits rounded to nearest;
    sin(idx) = cos(idx - 1024)"""
    idx = ((np.asarray(phase, np.int64) + 0x80000) & 0xffffffff) >> 20
    return _cos_of(idx), _cos_of((idx - 1024) & 4095)


def inc_of(f_hz):
    """uint32 phase increment per sample of a float32 frequency: rint of the double product, modulo 2^32."""
    return U32(int(np.rint(np.float64(F32(f_hz)) * (4294967296.0 / 12000.0))) & 0xffffffff)


def start_of(dt_s):
    """centre of the time search: rint((dt + 0.5) * 12000) in float32 (one add, one multiply), clamped to +-400000, minus CAND_OFFSET"""
    with np.errstate(all="ignore"):
        v = float(np.rint((F32(dt_s) + F32(0.5)) * F32(12000.0)))
    if not v >= -400000.0:
        v = -400000.0
    if v > 400000.0:
        v = 400000.0
    return int(v) - CAND_OFFSET


def phase_bases(tones, inc):
    """phase (uint32 turns) at the first sample of every symbol: what the increments of all symbols before add up to"""
    t = np.asarray(tones, np.int64)
    tp, tn = np.concatenate([t[:1], t[:-1]]), np.concatenate([t[1:], t[-1:]])
    per = NSPS * int(inc) + tp * int(CPT[2]) + t * int(CPT[1]) + tn * int(CPT[0])
    base = np.concatenate([[0], np.cumsum(per)[:-1]])
    return (base & 0xffffffff).astype(U32)


def wave(tones, inc):
    """cos, sin (float32[NW]) of the unit waveform: integer phase, table by its top 12 bits rounded to nearest"""
    t = np.asarray(tones, np.int64)
    tp, tn = np.concatenate([t[:1], t[:-1]]), np.concatenate([t[1:], t[-1:]])
    base = phase_bases(tones, inc).astype(np.int64)
    v = np.arange(NSPS, dtype=np.int64)
    ph = (base[:, None] + v[None, :] * int(inc) + tp[:, None] * CP[2].astype(np.int64)[None, :] + t[:, None] * CP[1].astype(np.int64)[None, :]
          + tn[:, None] * CP[0].astype(np.int64)[None, :]) & 0xffffffff
    return cos_sin(ph.reshape(-1))


def _padded(frame, start, lo, hi):
    """frame samples start+lo .. start+hi-1, +0 outside the frame"""
    out = np.zeros(hi - lo, F32)
    a, b = start + lo, start + hi
    ca, cb = max(a, 0), min(b, N)
    if cb > ca:
        out[ca - a:cb - a] = frame[ca:cb]
    return out


def block_sums(x, c, s):
    """x, c, s: float32[NW] -> (re, im) float32[NBLK]: re += x c, im -= x s over the block's 18 samples in ascending order"""
    x, c, s = x.reshape(NBLK, BLK), c.reshape(NBLK, BLK), s.reshape(NBLK, BLK)
    re, im = np.zeros(NBLK, F32), np.zeros(NBLK, F32)
    for i in range(BLK):
        re = re + x[:, i] * c[:, i]
        im = im - x[:, i] * s[:, i]
    return re, im


def halve32(a):
    """[..., 32] -> [...]: a[l] += a[l + h] for l < h, h = 16, 8, 4, 2, 1"""
    for h in (16, 8, 4, 2, 1):
        a = a[..., :h] + a[..., h:2 * h]
    return a[..., 0]


def symbol_metric(re, im):
    """[..., NBLK] block sums -> sum over the 103 symbols, ascending, of |symbol sum|^2"""
    sr, si = halve32(re.reshape(re.shape[:-1] + (NSYM, BPS))), halve32(im.reshape(im.shape[:-1] + (NSYM, BPS)))
    p = sr * sr + si * si
    m = np.zeros(p.shape[:-1], F32)
    for n in range(NSYM):
        m = m + p[..., n]
    return m


def first_max(m):
    best, arg = m[0], 0
    for i in range(1, len(m)):
        if m[i] > best:
            best, arg = m[i], i
    return arg


def tree256(terms):
    """terms float32[NBLK] -> thread l adds terms l, l + 256, .. ascending; then a[l] += a[l + h], h = 128 .. 1"""
    pad = np.zeros(NROWS * 256, F32)
    pad[:NBLK] = terms
    rows = pad.reshape(NROWS, 256)
    a = np.zeros(256, F32)
    for r in range(NROWS):
        a = a + rows[r]
    for h in (128, 64, 32, 16, 8, 4, 2, 1):
        a = a[:h] + a[h:2 * h]
    return a[0]


def freq_search(re, im):
    """index 0..52 of the first maximum over k = -26..26 of the symbol metric of the block sums turned back by k DINC (18 b + 9)"""
    k = np.arange(-KF, KF + 1, dtype=np.int64)
    u = BLK * np.arange(NBLK, dtype=np.int64) + BLK // 2
    rho = (k[:, None] * DINC * u[None, :]) & 0xffffffff
    cr, sr = cos_sin(rho)
    rre = re[None, :] * cr + im[None, :] * sr
    rim = im[None, :] * cr - re[None, :] * sr
    return first_max(symbol_metric(rre, rim))


def track(re, im, cnt):
    """amplitude track: Hann window over blocks b - 48 .. b + 48 inside the signal, ascending; normalised by the samples under the window"""
    pre, pim, pc = (np.concatenate([np.zeros(HW, F32), v, np.zeros(HW, F32)]) for v in (re, im, cnt))
    nre, nim, den = np.zeros(NBLK, F32), np.zeros(NBLK, F32), np.zeros(NBLK, F32)
    for j in range(2 * HW + 1):
        nre = nre + WIN[j] * pre[j:j + NBLK]
        nim = nim + WIN[j] * pim[j:j + NBLK]
        den = den + WIN[j] * pc[j:j + NBLK]
    ok = den > 0
    with np.errstate(all="ignore"):
        a_re = np.where(ok, nre / np.where(ok, den, F32(1)), F32(0)).astype(F32)
        a_im = np.where(ok, nim / np.where(ok, den, F32(1)), F32(0)).astype(F32)
    return a_re, a_im


SLOPE_K = 4294967296.0 / (6.283185307179586 * BLK)     # radians per block -> 2^-32 turns per sample


def slope_dinc(a_re, a_im):
    """integer correction of the increment from the track's mean turn per block: q = sum Im(a[b+1] conj a[b]) / sum Re(a[b+1] conj a[b]) (the
    small-angle tangent; both sums by the figures' tree over b = 0..NBLK-2), clamped to +-2 DINC -- the searches are trusted to two grid steps --
    and +0 where the denominator is not positive"""
    with np.errstate(all="ignore"):
        cr = np.zeros(NBLK, F32)
        ci = np.zeros(NBLK, F32)
        cr[:-1] = a_re[1:] * a_re[:-1] + a_im[1:] * a_im[:-1]
        ci[:-1] = a_im[1:] * a_re[:-1] - a_re[1:] * a_im[:-1]
        num, den = tree256(ci), tree256(cr)
        if not den > 0:
            return 0
        d = np.float64(num / den) * SLOPE_K
    if not d >= -2.0 * DINC:
        d = -2.0 * DINC
    if d > 2.0 * DINC:
        d = 2.0 * DINC
    return int(np.rint(d))


def fit(frame, tones, freq_hz, dt_s):
    """One decode against the ORIGINAL frame.  Returns (report record, fit dict with start, inc, tones, track a_re/a_im[NBLK])."""
    frame = np.asarray(frame, F32)
    inc0 = inc_of(freq_hz)
    i0 = start_of(dt_s)
    win = _padded(frame, i0, -TAU_MAX, NW + TAU_MAX)
    # frequency search at block rate: the block sums at the record's time and frequency, turned back by k DINC (18 b + 9)
    c, s = wave(tones, inc0)
    ik = freq_search(*block_sums(win[TAU_MAX:TAU_MAX + NW], c, s))
    inc = U32((int(inc0) + (ik - KF) * DINC) & 0xffffffff)
    # time search at the refined frequency, at sample rate
    c, s = wave(tones, inc)
    m = np.zeros(NTAU, F32)
    for it in range(NTAU):
        re, im = block_sums(win[it * TAU_STEP:it * TAU_STEP + NW], c, s)
        m[it] = symbol_metric(re, im)
    it = first_max(m)
    start = i0 - TAU_MAX + it * TAU_STEP
    # the frequency search once more, now that the symbols are aligned, and the block sums at the winner
    ik2 = freq_search(*block_sums(win[it * TAU_STEP:it * TAU_STEP + NW], c, s))
    inc = U32((int(inc) + (ik2 - KF) * DINC) & 0xffffffff)
    t = start + np.arange(NW, dtype=np.int64)
    cnt = ((t >= 0) & (t < N)).reshape(NBLK, BLK).sum(axis=1).astype(F32)
    c, s = wave(tones, inc)
    re, im = block_sums(win[it * TAU_STEP:it * TAU_STEP + NW], c, s)
    a_re, a_im = track(re, im, cnt)
    # the track's own phase slope, coherent over the whole signal: what the grid search left of the frequency turns the track from block to block
    inc = U32((int(inc) + slope_dinc(a_re, a_im)) & 0xffffffff)
    c, s = wave(tones, inc)
    re, im = block_sums(win[it * TAU_STEP:it * TAU_STEP + NW], c, s)
    a_re, a_im = track(re, im, cnt)
    with np.errstate(all="ignore"):
        # the figures, at block rate (energy of A cos = 2 |a|^2 per sample)
        okc = cnt > 0
        safe = np.where(okc, cnt, F32(1))
        removed = tree256(F32(2.0) * (a_re * a_re + a_im * a_im) * cnt)
        before = tree256(np.where(okc, F32(2.0) * (re * re + im * im) / safe, F32(0)).astype(F32))
        dr, di = re - cnt * a_re, im - cnt * a_im
        after = tree256(np.where(okc, F32(2.0) * (dr * dr + di * di) / safe, F32(0)).astype(F32))
    rec = np.zeros((), SUB_DTYPE)
    rec["f_hz"] = F32(np.float64(int(inc)) * (12000.0 / 4294967296.0))
    rec["dt_s"] = F32(start - 6000) / F32(12000.0)
    rec["p_removed"], rec["p_before"], rec["p_after"] = removed, before, after
    rec["n_inside"] = int(cnt.sum())
    rec["df_steps"], rec["dt_steps"] = (ik - KF) + (ik2 - KF), it - TAU_MAX // TAU_STEP
    return rec, {"start": start, "inc": inc, "tones": np.asarray(tones, np.int64), "a_re": a_re, "a_im": a_im}


def fitted_wave(f):
    """float32[NW]: y = a_re c - a_im s, the track interpolated linearly between block centres (held flat before the first and after the last)"""
    c, s = wave(f["tones"], f["inc"])
    p = 2 * np.arange(NW, dtype=np.int64) - (BLK - 1)
    b0 = np.clip(p // (2 * BLK), 0, NBLK - 2)
    m = p - 2 * BLK * b0
    g = m.astype(F32) * R36
    a0r, a1r, a0i, a1i = f["a_re"][b0], f["a_re"][b0 + 1], f["a_im"][b0], f["a_im"][b0 + 1]
    with np.errstate(all="ignore"):
        # before the first centre: a[0]; past the last: a[NBLK - 1]
        ar = np.where(m >= 2 * BLK, a1r, np.where(p < 0, a0r, a0r + g * (a1r - a0r))).astype(F32)
        ai = np.where(m >= 2 * BLK, a1i, np.where(p < 0, a0i, a0i + g * (a1i - a0i))).astype(F32)
        return ar * c - ai * s


def apply(frame, fits):
    """residual = frame - 2 y_d for every fit in order, on the samples of the signal that lie inside the frame"""
    out = np.array(frame, F32, copy=True)
    for f in fits:
        y = fitted_wave(f)
        a, b = max(f["start"], 0), min(f["start"] + NW, N)
        if b > a:
            out[a:b] = out[a:b] - F32(2.0) * y[a - f["start"]:b - f["start"]]
    return out


def subtract(frame, items):
    """items: (tones[103], f1_hz, dt_s) in emission order -> (reports SUB_DTYPE[n], residual float32[N], fits)"""
    fits, recs = [], np.zeros(len(items), SUB_DTYPE)
    for i, (tones, f, dt) in enumerate(items):
        recs[i], ft = fit(frame, tones, f, dt)
        fits.append(ft)
    return recs, apply(frame, fits), fits


def footprint_power(frame, f):
    """test-side measure: the energy of ANY frame along a fit's de-chirped track (what p_before is for the original frame)"""
    c, s = wave(f["tones"], f["inc"])
    re, im = block_sums(_padded(np.asarray(frame, F32), f["start"], 0, NW), c, s)
    t = f["start"] + np.arange(NW, dtype=np.int64)
    cnt = ((t >= 0) & (t < N)).reshape(NBLK, BLK).sum(axis=1).astype(np.float64)
    e = 2.0 * (re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2)
    return float(np.sum(e[cnt > 0] / cnt[cnt > 0]))
