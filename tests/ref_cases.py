"""The inputs of tests/test_oracle_vs_ref.py, shared with tests/gen_golden.py.

gen_golden.py runs them through the compiled reference headers (oracle/_ref) and records what the reference returned in
tests/golden/ref_*.npz; the test runs the oracle's restatement over the same inputs and compares bits with that record.
Every input is generated from a seed, so nothing but the recorded outputs is stored."""
import random

import numpy as np

DEMOD_CASES = [(192000, -26000, True), (192000, 90000, True), (192000, 12000, False),
               (96000, -30000, True), (48000, 9000, True), (48000, -3000, False)]
LOWPASS_CASES = ((512, 6000 / 192000.), (256, 6000 / 96000.), (128, 0.125))
BAD_DEMODS = ((192000, 97000.0), (192000, 93000.0), (44100, 0.0))
FRAMING_CASES = [("FT4", 48000, 1024, 3000), ("FT8", 96000, 2048, -20000), ("FT4", 192000, 2048, 50000)]
MODES = ["FT8", "JS8", "FT4", "WSPR", "Q65-30", "JT65", "FST4-60", "FST4-120", "FST4-300", "FST4-900", "FST4-1800",
         "FST4W-120", "FST4W-300", "FST4W-900", "FST4W-1800", "PSK31"]
TRIM_CORE = "123045 -12  0.3 1234 ~  CQ K1ABC FN42"


def demod_file(fs, f, usb):
    return f"ref_demod_fs{fs}_f{f}_{'usb' if usb else 'lsb'}.npz"


def demod_iq(O, fs, f, usb):
    D = fs // 12000
    return O.synth_iq(fs ^ (f & 0xFFFF), 4 * D * 3000, fs, tones_hz=[f + 1000.0, f - 1800.0 if not usb else f + 2222.0], amp=1e4)


def framing_file(mode, fs, blk, f):
    return f"ref_framing_{mode.lower()}_fs{fs}_b{blk}_f{f}.npz"


def framing_schedule(O, mode, fs, blk, f):
    """Random schedules of blocks and boundaries, including over-full slots ("af buffer full"), empty slots and the discarded first frame:
    [(blocks: complex64[n, blk], epoch)] for six slots."""
    rng = np.random.default_rng(fs + blk)
    cap_blocks = (O.frame_len(mode) - 1) // (blk // (fs // 12000))      # blocks a frame accepts before the guard trips
    epoch = 1000
    out = []
    for slot in range(6):
        n_blocks = [cap_blocks // 3, 0, cap_blocks + 5, 1, cap_blocks, 7][slot]
        iq = O.synth_iq(100 + slot, max(1, n_blocks) * blk, fs, tones_hz=[f + 1500.0], amp=8000.0)
        epoch += int(rng.integers(1, 20))
        out.append((iq[:n_blocks * blk].reshape(n_blocks, blk), epoch))
    return out


def helper_strings():
    """(locators, padded decode lines): the candidate locators of an FT8 'CQ K1ABC <loc>' line and TRIM_CORE with random padding."""
    rng = random.Random(5)
    alphabet = "ABfn0199 -/x"
    locs = []
    for _ in range(400):
        loc = "".join(rng.choice(alphabet) for _ in range(rng.choice([3, 4, 4, 4, 5])))
        if " " not in loc:
            locs.append(loc)
    padded = []
    for _ in range(200):
        pad_l = "".join(rng.choice(" \t") for _ in range(rng.randrange(0, 4)))
        pad_r = "".join(rng.choice(" \t\r\n") for _ in range(rng.randrange(0, 4)))
        padded.append(pad_l + TRIM_CORE + pad_r)
    return locs, padded


def tune_live_case(O):
    """SSBD::Tune(F, isUSB) mid-stream at 96 kHz: (fs, iq, first half's length, start, rejected retune, accepted retune)."""
    fs = 96000
    iq = O.synth_iq(3, 64 * 32 * 12, fs, tones_hz=[-20000 + 1000.0, 31000 + 1700.0], amp=9000.0)
    return fs, iq, 64 * 32 * 5, -20000, 45000, 31000


def tune_noreset_case(O):
    """SSBD::Tune(F, isUSB, reset = false) at 192 kHz through two retunes: (fs, iq, start, cuts, plan)."""
    fs = 192000
    iq = O.synth_iq(5, 64 * 40 * 9, fs, tones_hz=[-26000 + 900.0, 60000 + 1500.0, 1234 + 700.0], amp=9000.0)
    return fs, iq, -26000, [0, 64 * 40 * 3, 64 * 40 * 6, 64 * 40 * 9], [None, (60000, True), (1234, False)]
