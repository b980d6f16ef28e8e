"""Test helper: the numpy restatement of cwslg_ft4_soft (include/cwsl_gpu.h, "FT4 soft bits") -- float32 throughout, the fmaf chains, the
complex sums and the two 206-term trees written out as the header states them, not np.sum -- plus synthetic FT4 transmissions whose tones
are known.  PARITY UNPINNED like the rest of the sync stage: this is the repository's own statement of upstream ft4_decode's last stage
before LDPC (final downsample at f1, get_ft4_bitmetrics, nsync / nqual, normalizebmet).

Input: cb = oracle.ft4_downsample(cx, f1_hz)[0] per record (the baseband the header defines by reference to orc_ft4_downsample) and ibest."""
import numpy as np

from ft8_signal import ICOS4, ft4_frame_tones

F32 = np.float32
NN, NSS, NP, NBM, NBIT = 103, 32, 4032, 206, 174
RECORD_BYTES = 2112
GRAYMAP = np.array([0, 1, 3, 2])
COSTAS_SYMBOLS = np.array([33 * b + s for b in range(4) for s in range(4)])
DATA_SYMBOLS = np.array(list(range(4, 33)) + list(range(37, 66)) + list(range(70, 99)))          # 87 data symbols, 2 bits each
LLR_ENTRIES = np.concatenate([np.arange(8, 66), np.arange(74, 132), np.arange(140, 198)])        # = 2 * DATA_SYMBOLS + (0, 1)
QUAL_AT = np.concatenate([np.arange(0, 8), np.arange(66, 74), np.arange(132, 140), np.arange(198, 206)])
QUAL_BITS = np.array([0, 0, 0, 1, 1, 0, 1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1])


def _w32():
    p = np.arange(32)
    w = np.stack([np.cos(2.0 * np.pi * p / 32.0).astype(F32), np.sin(2.0 * np.pi * p / 32.0).astype(F32)], axis=1)
    w[0], w[8], w[16], w[24] = (1, 0), (0, 1), (-1, 0), (0, -1)
    return w


W32 = _w32()


def fmaf(a, b, c):
    """Correctly rounded float32 fused multiply-add of float32 arrays: the product of two float32 is exact in float64; the float64 sum is made
    'round to odd' with the error term of TwoSum, after which the rounding to float32 is the single rounding of a true fmaf."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even & np.isfinite(s)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def mag(zr, zi):
    """|z| = sqrtf(fmaf(z.r, z.r, z.i * z.i))"""
    return np.sqrt(fmaf(zr, zr, zi * zi), dtype=F32)


def symbols(cb, ibest):
    """cd[q, k, t] = cb[q, ibest[q] + 32 k + t], +0 outside 0..4031 -> (re, im) float32[q, 103, 32]"""
    cb = np.ascontiguousarray(cb, dtype=np.complex64).reshape(-1, NP)
    ib = np.asarray(ibest, np.int64).reshape(-1, 1)
    idx = ib + np.arange(NN * NSS).reshape(1, -1)
    ok = (idx >= 0) & (idx < NP)
    v = cb[np.arange(cb.shape[0]).reshape(-1, 1), np.clip(idx, 0, NP - 1)]
    re = np.where(ok, v.real, F32(0)).astype(F32).reshape(-1, NN, NSS)
    im = np.where(ok, v.imag, F32(0)).astype(F32).reshape(-1, NN, NSS)
    return re, im


def symbol_spectra(cb, ibest):
    """cs[q, k, tone] as (re, im) float32[q, 103, 4]: the 32-term fmaf chain in ascending t"""
    re, im = symbols(cb, ibest)
    zr = np.zeros(re.shape[:2] + (4,), F32)
    zi = np.zeros_like(zr)
    tone = np.arange(4)
    for t in range(NSS):
        w = W32[(tone * t) % 32]
        wx, wy = w[:, 0].reshape(1, 1, 4), w[:, 1].reshape(1, 1, 4)
        cr, ci = re[:, :, t:t + 1], im[:, :, t:t + 1]
        zr = fmaf(cr, wx, zr); zr = fmaf(ci, wy, zr)
        zi = fmaf(ci, wx, zi); zi = fmaf(-cr, wy, zi)
    return zr, zi


def _metrics(s2, nb):
    """s2 float32[..., 2^nb] -> float32[..., nb]: metric ib = max(s2[i] : bit nb-1-ib of i set) - max(s2[i] : clear)"""
    i = np.arange(1 << nb)
    out = []
    for ib in range(nb):
        on = ((i >> (nb - 1 - ib)) & 1) == 1
        out.append(s2[..., on].max(axis=-1) - s2[..., ~on].max(axis=-1))
    r = np.stack(out, axis=-1)
    assert r.dtype == F32
    return r


def bitmetrics(cb, ibest):
    """-> dict(cs=(re, im), mag float32[q, 103, 4], bm float32[q, 3, 206] (un-normalised, tail copies in place), nsync, nqual int32[q])"""
    zr, zi = symbol_spectra(cb, ibest)
    n = zr.shape[0]
    m = mag(zr, zi)
    want = np.array(ICOS4).reshape(1, 16)
    nsync = (np.argmax(m[:, COSTAS_SYMBOLS, :], axis=2) == want).sum(axis=1).astype(np.int32)       # np.argmax: the first maximum
    g = GRAYMAP
    bm = np.zeros((n, 3, NBM), F32)
    bm[:, 0, :] = _metrics(m[:, :, g], 2).reshape(n, NBM)
    # set 1: pairs
    ks = np.arange(0, 102, 2)
    i = np.arange(16)
    ar, ai = zr[:, ks][:, :, g[i >> 2]], zi[:, ks][:, :, g[i >> 2]]
    br, bi = zr[:, ks + 1][:, :, g[i & 3]], zi[:, ks + 1][:, :, g[i & 3]]
    bm[:, 1, :204] = _metrics(mag(ar + br, ai + bi), 4).reshape(n, 204)
    bm[:, 1, 204:206] = bm[:, 0, 204:206]
    # set 2: groups of four, ((a + b) + c) + d
    ks = np.arange(0, 100, 4)
    i = np.arange(256)
    sel = [g[i >> 6], g[(i >> 4) & 3], g[(i >> 2) & 3], g[i & 3]]
    sr, si = zr[:, ks][:, :, sel[0]], zi[:, ks][:, :, sel[0]]
    for j in (1, 2, 3):
        sr = sr + zr[:, ks + j][:, :, sel[j]]
        si = si + zi[:, ks + j][:, :, sel[j]]
    assert sr.dtype == F32
    bm[:, 2, :200] = _metrics(mag(sr, si), 8).reshape(n, 200)
    bm[:, 2, 200:204] = bm[:, 1, 200:204]
    bm[:, 2, 204:206] = bm[:, 0, 204:206]
    hard = (bm[:, 0, QUAL_AT] >= 0).astype(np.int64)
    nqual = (hard == QUAL_BITS.reshape(1, 32)).sum(axis=1).astype(np.int32)
    return dict(cs=(zr, zi), mag=m, bm=bm, nsync=nsync, nqual=nqual)


def _tree(x):
    """x float32[..., 206] -> float32[...]: pad to 256 with +0, a[l] = ((x[l] + x[l+64]) + x[l+128]) + x[l+192], then a[l] += a[l+h], h = 32 .. 1"""
    pad = np.zeros(x.shape[:-1] + (256,), F32)
    pad[..., :NBM] = x
    a = ((pad[..., 0:64] + pad[..., 64:128]) + pad[..., 128:192]) + pad[..., 192:256]
    h = 32
    while h >= 1:
        a = a[..., :h] + a[..., h:2 * h]
        h //= 2
    assert a.dtype == F32
    return a[..., 0]


def normalise(bm):
    """bm float32[q, 3, 206] -> (llr float32[q, 3, 174], sigma float32[q, 3])"""
    bm = np.asarray(bm, F32)
    s1, s2 = _tree(bm), _tree(bm * bm)
    mean, m2 = s1 / F32(206), s2 / F32(206)
    var = m2 - mean * mean
    sigma = np.sqrt(np.where(var > 0, var, m2).astype(F32), dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        llr = (bm[..., LLR_ENTRIES] / sigma[..., None]) * F32(2.83)
    llr = np.where(sigma[..., None] == 0, F32(0), llr).astype(F32)
    return llr, sigma


def softbits(cb, ibest):
    """cb complex64[q, 4032] (the baseband at each record's f1_hz), ibest int[q] -> (llr [q, 3, 174], sigma [q, 3], nsync [q], nqual [q])"""
    if len(np.atleast_1d(ibest)) == 0:
        return np.zeros((0, 3, NBIT), F32), np.zeros((0, 3), F32), np.zeros(0, np.int32), np.zeros(0, np.int32)
    r = bitmetrics(cb, ibest)
    llr, sigma = normalise(r["bm"])
    return llr, sigma, r["nsync"], r["nqual"]


def softbits_of_records(oracle, cx, recs):
    """The records of fetch_ft4_sync / oracle.ft4_sync_all on the frame spectrum cx (oracle.ft4_bigspec)."""
    cb = np.zeros((len(recs), NP), np.complex64)
    for q, r in enumerate(recs):
        cb[q] = oracle.ft4_downsample(cx, F32(r["f1_hz"]))[0]
    return softbits(cb, [r["ibest"] for r in recs])


def tone_bits(tones):
    """The 174 transmitted bits of 103 channel tones: per data symbol the v with graymap[v] == tone, MSB first."""
    inv = np.argsort(GRAYMAP)
    v = inv[np.asarray(tones)[DATA_SYMBOLS]]
    return np.stack([(v >> 1) & 1, v & 1], axis=1).reshape(NBIT)


def _phase(tones, f0_hz, sps, fs):
    f = f0_hz + (12000.0 / 576.0) * np.repeat(tones, sps)
    return 2 * np.pi * np.cumsum(f) / fs


def ft4_iq_with_tones(fs, n, rf_hz, audio_hz, t0_s, amp, seed):
    """Complex IQ of one FT4 transmission (Costas blocks at symbols 0 / 33 / 66 / 99, data from default_rng(seed)), tone 0 at rf_hz + audio_hz,
    first symbol t0_s into the buffer; t0_s < 0: the transmission began before the buffer and its leading samples are cut.  -> (iq, tones)"""
    tones = ft4_frame_tones(np.random.default_rng(seed))
    ph = _phase(tones, rf_hz + audio_hz, int(round(fs * 0.048)), fs)
    out = np.zeros(n, np.complex64)
    i0 = int(round(t0_s * fs))
    cut = max(0, -i0)
    m = min(len(ph) - cut, n - max(i0, 0))
    out[max(i0, 0):max(i0, 0) + m] = amp * np.exp(1j * ph[cut:cut + m])
    return out, tones


def ft4_frame(bursts, noise_sigma, seed, n=90000):
    """Real 12 kHz int16 frame of FT4 transmissions in Gaussian noise.  bursts: (f0_hz, t0_s, amp, tone_seed); t0_s may be negative.
    -> (frame, [tones per burst])"""
    x = np.random.default_rng(seed).normal(0.0, noise_sigma, n) if noise_sigma > 0 else np.zeros(n)
    all_tones = []
    for f0, t0, amp, ts in bursts:
        tones = ft4_frame_tones(np.random.default_rng(ts))
        ph = _phase(tones, f0, 576, 12000.0)
        i0 = int(round(t0 * 12000))
        cut = max(0, -i0)
        m = min(len(ph) - cut, n - max(i0, 0))
        x[max(i0, 0):max(i0, 0) + m] += amp * np.cos(ph[cut:cut + m])
        all_tones.append(tones)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16), all_tones
