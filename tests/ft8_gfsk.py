"""A GFSK FT8 synthesiser in float64 for test inputs: the protocol's waveform (BT = 2.0, h = 1, 6.25 Bd, 12 kHz) from first principles.  It
shares nothing with the subtractor's restatement (tests/ft8_subtract_ref.py): no table, no integer phase.  The phase is integrated on a grid
OS times finer than the sample grid, so a transmission may start between samples."""
import math

import numpy as np

FS = 12000.0
NSPS = 1920
NSYM = 79
N = 180000
OS = 4


def gfsk_pulse(bt, nsps):
    """frequency pulse of one symbol over three symbol times: a rectangle through a Gaussian filter"""
    c = math.pi * math.sqrt(2.0 / math.log(2.0))
    t = (np.arange(3 * nsps, dtype=np.float64) - 1.5 * nsps) / nsps
    erf = np.vectorize(math.erf)
    return 0.5 * (erf(c * bt * (t + 0.5)) - erf(c * bt * (t - 0.5)))


_PULSE = {}


def phase_track(tones, f_hz, os=OS):
    """phase in radians at the os-times oversampled instants of the 79 symbols, zero at the first"""
    nsps = NSPS * os
    if os not in _PULSE:
        _PULSE[os] = gfsk_pulse(2.0, nsps)
    pulse = _PULSE[os]
    tones = np.asarray(tones, np.float64)
    dphi = np.zeros((NSYM + 2) * nsps, np.float64)
    peak = 2.0 * math.pi / nsps
    for j in range(NSYM):
        dphi[j * nsps:(j + 3) * nsps] += peak * pulse * tones[j]
    dphi[:2 * nsps] += peak * tones[0] * pulse[nsps:]               # the first and last tone are held outside the transmission
    dphi[NSYM * nsps:] += peak * tones[-1] * pulse[:2 * nsps]
    dphi = dphi[nsps:(NSYM + 1) * nsps] + 2.0 * math.pi * f_hz / (FS * os)
    return np.concatenate([[0.0], np.cumsum(dphi)[:-1]])


def synth(tones, f_hz, dt_s, amp=1.0, phase0=0.0, n=N, os=OS):
    """float64[n]: amp cos(phase) of a transmission whose first symbol starts dt_s + 0.5 s into the frame (rounded to 1 / os sample), cut by
    the frame's edges; constant envelope"""
    ph = phase_track(tones, f_hz, os)
    k0 = int(round((dt_s + 0.5) * FS * os))          # start on the oversampled grid
    out = np.zeros(n, np.float64)
    # frame sample t sits at oversampled index t os - k0 of the track
    t_lo = max(0, -(-k0 // os))
    t_hi = min(n, (k0 + ph.size - 1) // os + 1)
    if t_hi > t_lo:
        idx = np.arange(t_lo, t_hi) * os - k0
        out[t_lo:t_hi] = amp * np.cos(ph[idx] + phase0)
    return out
