"""Removal depth of the FT4 subtractor as a MEASURED property: for a dozen noise-free and noisy frames, the energy left in the
signal's footprint after / before subtraction, for the float32 restatement (tests/ft4_subtract_ref.py: integer phase, committed tables) and for an
independent float64 implementation of the same statement below (np.cos, no tables, the pulse from first principles).  Run as a script it writes
profiles/ft4_subtract_quality.json; tests/test_ft4_subtract_ref.py calls measure() and holds the float32 figures to the float64 ones."""
import json
import math
import os
import sys

import numpy as np

import ft4_gfsk as G
import ft4_subtract_cases as SC
import ft4_subtract_ref as S

N, NSPS, NSYM, NW, BLK, NBLK = S.N, S.NSPS, S.NSYM, S.NW, S.BLK, S.NBLK


# ---- the statement in float64 ---------------------------------------------------------------------------------------------------------------------------
def wave64(tones, f_hz):
    ph = G.phase_track(tones, f_hz, os=1)
    return np.cos(ph), np.sin(ph)


def _padded64(frame, start):
    out = np.zeros(NW)
    a, b = max(start, 0), min(start + NW, N)
    if b > a:
        out[a - start:b - start] = frame[a:b]
    return out


def _blocks64(x, c, s):
    return (x * c).reshape(NBLK, BLK).sum(axis=1) - 1j * (x * s).reshape(NBLK, BLK).sum(axis=1)


def _metric64(B):
    return float((np.abs(B.reshape(B.shape[:-1] + (NSYM, S.BPS)).sum(axis=-1)) ** 2).sum(axis=-1)) if B.ndim == 1 else \
        (np.abs(B.reshape(B.shape[:-1] + (NSYM, S.BPS)).sum(axis=-1)) ** 2).sum(axis=-1)


def fit64(frame, tones, freq_hz, dt_s):
    """the same grids, window and order of steps; float64 throughout"""
    frame = np.asarray(frame, np.float64)
    i0 = int(np.rint((dt_s + 0.5) * 12000.0)) - S.CAND_OFFSET
    df = S.FREQ_STEP_HZ
    c, s = wave64(tones, freq_hz)
    B = _blocks64(_padded64(frame, i0), c, s)
    k = np.arange(-S.KF, S.KF + 1)
    u = float(BLK) * np.arange(NBLK) + BLK / 2.0
    rot = np.exp(-2j * np.pi * (k[:, None] * df) * u[None, :] / 12000.0)
    f = freq_hz + k[int(np.argmax(_metric64(B[None, :] * rot)))] * df
    c, s = wave64(tones, f)
    m = [_metric64(_blocks64(_padded64(frame, i0 - S.TAU_MAX + S.TAU_STEP * j), c, s)) for j in range(S.NTAU)]
    start = i0 - S.TAU_MAX + S.TAU_STEP * int(np.argmax(m))
    B = _blocks64(_padded64(frame, start), c, s)
    f = f + k[int(np.argmax(_metric64(B[None, :] * rot)))] * df              # the frequency once more, the symbols aligned
    c, s = wave64(tones, f)
    B = _blocks64(_padded64(frame, start), c, s)
    t = start + np.arange(NW)
    cnt = ((t >= 0) & (t < N)).reshape(NBLK, BLK).sum(axis=1).astype(np.float64)
    w = 0.5 * (1.0 + np.cos(np.pi * np.arange(-S.HW, S.HW + 1) / (S.HW + 1)))
    den = np.convolve(cnt, w, "same")

    def track64(B):
        return np.where(den > 0, np.convolve(B, w, "same") / np.where(den > 0, den, 1.0), 0.0)
    a = track64(B)
    # the track's mean turn per block (small-angle tangent), clamped to two grid steps; the block sums and the track once more
    z = np.sum(a[1:] * np.conj(a[:-1]))
    if z.real > 0:
        f = f + float(np.clip(z.imag / z.real / (2.0 * np.pi * BLK) * 12000.0, -2.0 * df, 2.0 * df))
        c, s = wave64(tones, f)
        B = _blocks64(_padded64(frame, start), c, s)
        a = track64(B)
    return {"start": start, "f": f, "tones": tones, "a": a}


def apply64(frame, fits):
    out = np.array(frame, np.float64)
    for f in fits:
        c, s = wave64(f["tones"], f["f"])
        centres = float(BLK) * np.arange(NBLK) + (BLK - 1) / 2.0
        uu = np.arange(NW, dtype=np.float64)
        ar, ai = np.interp(uu, centres, f["a"].real), np.interp(uu, centres, f["a"].imag)
        y = 2.0 * (ar * c - ai * s)
        a, b = max(f["start"], 0), min(f["start"] + NW, N)
        if b > a:
            out[a:b] -= y[a - f["start"]:b - f["start"]]
    return out


def footprint64(frame, truth):
    """energy of a frame along the TRUE transmission's de-chirped track (float64 waveform at the true f and start): the same yardstick for both"""
    tones, f_hz, dt_s = truth
    start = int(round((dt_s + 0.5) * 12000.0))
    c, s = wave64(tones, f_hz)
    B = _blocks64(_padded64(np.asarray(frame, np.float64), start), c, s)
    t = start + np.arange(NW)
    cnt = ((t >= 0) & (t < N)).reshape(NBLK, BLK).sum(axis=1).astype(np.float64)
    return float(np.sum(2.0 * np.abs(B[cnt > 0]) ** 2 / cnt[cnt > 0]))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------------------
# (word, true f_hz, true dt_s, amplitude, noise sigma): off the grids, on them (2000 Hz; 0.202 s is baseband sample 468), cut by either edge of
# the frame, then the same six in noise from strong to weak -- the twelve kinds of frame DESIGN.md 4.15 uses
CASES = [(0, 1234.56, 0.1237, 1000.0, 0.0), (1, 801.3, -0.31, 1000.0, 0.0), (2, 1500.9, 0.413, 1000.0, 0.0), (3, 2000.0, 0.202, 1000.0, 0.0),
         (4, 700.7, -0.62, 1000.0, 0.0), (5, 1900.2, 0.7, 1000.0, 0.0),
         (0, 1234.56, 0.1237, 1000.0, 100.0), (1, 801.3, -0.31, 1000.0, 300.0), (2, 1500.9, 0.413, 1000.0, 1000.0), (3, 2000.0, 0.202, 1000.0, 3000.0),
         (4, 700.7, -0.62, 1000.0, 1000.0), (5, 1900.2, 0.7, 1000.0, 3000.0)]


def measure():
    """-> [dict(case..., db32, db64)]: 10 log10(footprint energy after / before) of the float32 restatement and of the float64 implementation"""
    out = []
    for i, (k, f, dt, amp, sigma) in enumerate(CASES):
        tones = SC.tones(SC.word(k))
        x = SC.tx(k, f, dt, amp, 0.3 + i) + (SC.noise(100 + i, sigma) if sigma else 0.0)
        fg, dtg = SC.grid(f, dt)
        truth = (tones, f, dt)
        before = footprint64(x, truth)
        x32 = x.astype(np.float32)
        _, res32, _ = S.subtract(x32, [(tones, fg, dtg)])
        res64 = apply64(x, [fit64(x, tones, float(np.float32(fg)), float(np.float32(dtg)))])
        out.append(dict(word=k, f_hz=f, dt_s=dt, amp=amp, sigma=sigma, db32=10 * math.log10(footprint64(res32, truth) / before),
                        db64=10 * math.log10(footprint64(res64, truth) / before)))
    return out


if __name__ == "__main__":
    rows = measure()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "ft4_subtract_quality.json")
    diffs = [r["db32"] - r["db64"] for r in rows]
    with open(path, "w") as fh:
        fh.write('{"what": "footprint energy after / before subtraction, dB: float32 restatement (db32) and float64 implementation (db64)",\n "cases": [\n')
        fh.write(",\n".join("  " + json.dumps({k: (round(v, 3) if k.startswith("db") else v) for k, v in r.items()}) for r in rows))
        fh.write('],\n "db32_minus_db64": %s}\n' % json.dumps({"min": round(min(diffs), 4), "max": round(max(diffs), 4), "mean": round(sum(diffs) / len(diffs), 4)}))
    for r in rows:
        print(r)
    print(min(diffs), max(diffs))
