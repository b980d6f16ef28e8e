"""Test helper: the numpy restatement of cwslg_ft8_soft (include/cwsl_gpu.h, "FT8 soft bits") -- float32 throughout, the two 174-term
sums written out as the tree the header states -- plus synthetic FT8 frames whose transmitted tones are known.  PARITY UNPINNED like the
rest of the sync stage: this is the repository's own statement of upstream ft8b's nsym = 1 bit metrics on the symbol-spectra grid."""
import numpy as np

from ft8_signal import ICOS7, ft8_iq, ft8_tones

F32 = np.float32
GRAYMAP = np.array([0, 1, 3, 2, 5, 6, 4, 7])
DATA_SYMBOLS = np.array(list(range(7, 36)) + list(range(43, 72)))          # 58 data symbols, 3 bits each
COSTAS_SYMBOLS = np.array([base + r for base in (0, 36, 72) for r in range(7)])
NHSYM, NH1 = 372, 1920


def soft_pitch(f_hi_hz):
    """Row pitch of the plane while the feature is on: ib + 15 rounded up to 32 bins (ib as cwslg_enable_sync derives it)."""
    ib = min(int(np.floor(F32(f_hi_hz) / F32(3.125) + F32(0.5))), NH1 - 12)
    return (ib + 15 + 31) // 32 * 32


def magnitudes(spectra, cands):
    """s8[q, n, k] = sqrtf(S(i + 2k, j + 12 + 4n)); 0 where the step is outside 1..372 or the bin above 1920.  cands: (freq_bin, time_step, ...)."""
    sp = np.ascontiguousarray(spectra, dtype=F32)
    assert sp.shape[0] == NHSYM
    i = np.array([c[0] for c in cands], np.int64).reshape(-1, 1, 1)
    j = np.array([c[1] for c in cands], np.int64).reshape(-1, 1, 1)
    m = j + 12 + 4 * np.arange(79).reshape(1, -1, 1)                      # 1-based step
    b = i + 2 * np.arange(8).reshape(1, 1, -1)
    ok = (m >= 1) & (m <= NHSYM) & (b <= NH1)
    assert np.minimum(b, NH1).max() < sp.shape[1], "row pitch does not hold tone 7"
    mm = np.clip(m - 1, 0, NHSYM - 1)
    bb = np.clip(b, 0, sp.shape[1] - 1)
    p = np.where(ok, sp[mm, bb], F32(0))
    return np.sqrt(p.astype(F32), dtype=F32)


def _tree(x):
    """x float32[q, 174] -> float32[q]: pad to 192 with +0, a[l] = (x[l] + x[l+64]) + x[l+128], then a[l] += a[l+h] for h = 32 .. 1."""
    pad = np.zeros((x.shape[0], 192), F32)
    pad[:, :174] = x
    a = (pad[:, 0:64] + pad[:, 64:128]) + pad[:, 128:192]
    h = 32
    while h >= 1:
        a = a[:, :h] + a[:, h:2 * h]
        h //= 2
    assert a.dtype == F32
    return a[:, 0]


def softbits(spectra, cands):
    """-> (llr float32[q, 174], sigma float32[q], nsync int32[q]) of the candidates (freq_bin, time_step, ...) on the plane `spectra` [372, pitch]."""
    if len(cands) == 0:
        return np.zeros((0, 174), F32), np.zeros(0, F32), np.zeros(0, np.int32)
    s8 = magnitudes(spectra, cands)
    # nsync: first maximum (np.argmax: ties to the lowest tone, Fortran maxloc) against icos7
    nsync = (np.argmax(s8[:, COSTAS_SYMBOLS, :], axis=2) == np.array(ICOS7 * 3).reshape(1, -1)).sum(axis=1).astype(np.int32)
    s2 = s8[:, DATA_SYMBOLS, :][:, :, GRAYMAP]                            # s2[v] = s8[graymap[v]]
    mx = lambda idx: s2[:, :, idx].max(axis=2)
    b = np.stack([mx([4, 5, 6, 7]) - mx([0, 1, 2, 3]),
                  mx([2, 3, 6, 7]) - mx([0, 1, 4, 5]),
                  mx([1, 3, 5, 7]) - mx([0, 2, 4, 6])], axis=2).reshape(-1, 174)
    assert b.dtype == F32
    s1, sq = _tree(b), _tree(b * b)
    mean, m2 = s1 / F32(174), sq / F32(174)
    var = m2 - mean * mean
    sigma = np.sqrt(np.where(var > 0, var, m2).astype(F32), dtype=F32)
    with np.errstate(divide="ignore", invalid="ignore"):
        llr = (b / sigma.reshape(-1, 1)) * F32(2.83)
    llr = np.where(sigma.reshape(-1, 1) == 0, F32(0), llr).astype(F32)
    return llr, sigma, nsync


def tone_bits(tones):
    """The 174 transmitted bits of 79 channel tones: per data symbol the v with graymap[v] == tone, MSB first."""
    inv = np.argsort(GRAYMAP)
    v = inv[np.asarray(tones)[DATA_SYMBOLS]]
    return np.stack([(v >> 2) & 1, (v >> 1) & 1, v & 1], axis=1).reshape(174)


def symbols_past_end(lag):
    """Mask[174] of the bits whose symbol lies past step 372 for a candidate at this lag."""
    past = (lag + 12 + 4 * DATA_SYMBOLS) > NHSYM
    return np.repeat(past, 3)


def ft8_frame(f0_hz, t0_s, amp, noise_sigma, seed, n=240000, n_valid=180000):
    """Real 12 kHz int16 frame (n samples, zero from n_valid on) of one FT8 transmission, tone 0 at f0_hz, first symbol t0_s into the frame, in
    Gaussian noise.  The tones come from ft8_tones(default_rng(seed)), the noise from the same generator after them.  -> (frame, tones)."""
    rng = np.random.default_rng(seed)
    tones = ft8_tones(rng)
    noise = rng.normal(0.0, noise_sigma, n)
    f = f0_hz + 6.25 * np.repeat(tones, 1920)
    ph = 2 * np.pi * np.cumsum(f) / 12000.0
    x = noise
    i0 = int(round(t0_s * 12000))
    k = min(len(ph), n - i0)
    x[i0:i0 + k] += amp * np.cos(ph[:k])
    x[n_valid:] = 0.0
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16), tones


def ft8_iq_with_tones(fs, n, rf_hz, audio_hz, t0_s, amp, seed):
    """ft8_signal.ft8_iq of default_rng(seed) together with the tones it transmits (a twin generator draws them again)."""
    tones = ft8_tones(np.random.default_rng(seed))
    return ft8_iq(fs, n, rf_hz, audio_hz, t0_s, amp, np.random.default_rng(seed)), tones
