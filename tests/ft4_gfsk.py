"""A GFSK FT4 synthesiser in float64 for test inputs: the protocol's waveform (BT = 1.0, h = 1, 20.8333 Bd, 12 kHz) from first principles, on
ft8_gfsk's frequency pulse.  It shares nothing with the subtractor's restatement (tests/ft4_subtract_ref.py): no table, no integer phase.  The 103
channel symbols alone, constant envelope: the protocol's two ramp symbols are not made, as the subtractor does not model them.  The phase is
integrated on a grid OS times finer than the sample grid, so a transmission may start between samples."""
import math

import numpy as np

import ft8_gfsk as G8

FS = 12000.0
NSPS = 576
NSYM = 103
N = 72576
OS = 4

_PULSE = {}


def phase_track(tones, f_hz, os=OS):
    """phase in radians at the os-times oversampled instants of the 103 symbols, zero at the first"""
    nsps = NSPS * os
    if os not in _PULSE:
        _PULSE[os] = G8.gfsk_pulse(1.0, nsps)
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
