"""Further inputs of the FT4 subtractor's flat call (tests/test_subtract_edge_inputs.py proves on the CPU what each one contains;
tests/test_gpu_ft4_subtract_kernel.py runs them on the device): starts off the 18-sample baseband grid, so that the window's alignment remainder
w0 mod 4 of modules/ft4sub.hip's sub_tile_pass is 1 and 3 as well as 0 and 2 and the padded-word select runs on odd r0; items at the limits the
host accepts; a table of offsets with runs of equal entries and one frame with 24 items; that frame with its items in reverse order.  Built with
tests/ft4_subtract_cases.py's helpers; every reference is computed once and shared."""
import functools

import numpy as np

import ft4_subtract_ref as S
from ft4_subtract_cases import ITEM_DTYPE, SEED, item, noise, tones, tx, word  # noqa: F401  (word: for the tests)

N = S.N
FS = 12000.0
TONE_HZ = 12000.0 / 576.0
NAMES = ("offgrid", "limits", "crowded", "reversed", "trailing")


def at(frame, k, freq_hz, i0):
    """an item whose dt_s is `i0` / 12000 - 0.5: the start the kernel derives is i0"""
    return item(frame, k, freq_hz, np.float32(i0 / FS - 0.5))


def sent(k, f_hz, first, amp, phase0=0.0):
    """the transmission of word k whose first sample is `first`"""
    return tx(k, f_hz, first / FS - 0.5, amp, phase0)


# offgrid: (word, true frequency, the item's start i0, true first sample minus i0, amplitude).  The window of tile 0 starts at w0 = i0 - 54, so
# w0 mod 4 is (i0 + 2) mod 4: 0, 1, 2, 3; on the second and the fourth r is odd, and r0 = (r + 2 it) mod 18 with it.  The time grid has 2
# samples: the four starts are 0, +11, -7 and +3 samples from i0, and the restatement's winners are -1, 8, -3 and 2 steps.
OFFGRID = ((20, 700.3, 7202, 0, 600.0), (21, 1333.3, 3003, 11, 500.0), (22, 1999.1, 9600, -7, 700.0), (23, 2600.7, 5401, 3, 400.0))
# limits: the items in front of the real transmission (word, frequency, dt_s): both ends of dt_s; a window whose earliest offset leaves the last 10
# samples of the frame to the signal's first block; one whose latest offset leaves the frame's first 10 samples to the signal's last block; both
# ends of freq_hz (the word at 0 Hz is one whose search goes below 0 in this frame's noise)
SLIVER_END = (N - 10 + S.TAU_MAX) / FS - 0.5
SLIVER_START = (10 - S.NW - S.TAU_MAX) / FS - 0.5
LIMITS = ((31, 1000.0, 30.0), (32, 1000.0, -30.0), (33, 1500.0, SLIVER_END), (34, 1500.0, SLIVER_START), (38, 0.0, 0.02), (36, 6000.0, 0.02))
LIMITS_TX = (30, 1750.0, 7200, 800.0)
# crowded, frame 3: twelve transmissions (word, frequency, first sample, amplitude); the first four are pairwise within one tone spacing
# (20.83 Hz) and overlap in time
CROWD = ((40, 1000.0, 6000, 500.0), (41, 1007.0, 6600, 450.0), (42, 1014.0, 5400, 400.0), (43, 1019.5, 7200, 550.0),
         (44, 400.0, 1200, 300.0), (45, 650.0, 3000, 350.0), (46, 1300.0, 8001, 600.0), (47, 1600.0, 9602, 250.0),
         (48, 1900.0, 11003, 700.0), (49, 2200.0, 2401, 320.0), (50, 2500.0, 12000, 380.0), (51, 2800.0, 13001, 420.0))
CROWD_COUNTS = {0: 1, 3: 24, 7: 2}
CROWD_FRAMES = 8


def grid_hz(f_hz):
    return float(round(f_hz))


def _crowd_frame():
    return sum(sent(k, f, s, a, 0.37 * i) for i, (k, f, s, a) in enumerate(CROWD)) + noise(43, 120.0)


def _crowd_items(frame):
    """each of the twelve named twice: as a record would carry it, then 1 Hz and 3 samples away"""
    first = [at(frame, k, grid_hz(f), s) for k, f, s, a in CROWD]
    second = [at(frame, k, grid_hz(f) + 1.0, s + 3) for k, f, s, a in CROWD]
    return first + second


@functools.lru_cache(maxsize=None)
def kernel_cases():
    """name -> (audio float32 [n_frames][N], items ITEM_DTYPE[n])"""
    out = {}
    a = sum(sent(k, f, s + d, amp, 0.9 * i) for i, (k, f, s, d, amp) in enumerate(OFFGRID)) + noise(31, 150.0)
    out["offgrid"] = (a[None, :], [at(0, k, grid_hz(f), s) for k, f, s, d, amp in OFFGRID])
    k, f, s, amp = LIMITS_TX
    a = sent(k, f, s, amp, 0.4) + noise(32, 200.0)
    out["limits"] = (a[None, :], [item(0, w, fq, np.float32(d)) for w, fq, d in LIMITS] + [at(0, k, grid_hz(f), s)])
    frames = [noise(40 + i, 100.0 + 10.0 * i) for i in range(CROWD_FRAMES)]
    frames[0] = frames[0] + sent(60, 900.0, 6480, 500.0)
    frames[3] = _crowd_frame()
    frames[7] = frames[7] + sent(61, 1200.0, 5040, 400.0) + sent(62, 2000.0, 8405, 600.0, 1.0)
    out["crowded"] = (np.stack(frames), [at(0, 60, grid_hz(900.0), 6480)] + _crowd_items(3) + [at(7, 61, grid_hz(1200.0), 5040), at(7, 62, grid_hz(2000.0), 8405)])
    out["reversed"] = (frames[3][None, :], _crowd_items(0)[::-1])
    # three frames, the last two without an item: the tail of the offsets table is filled on more than one frame
    out["trailing"] = (np.stack([frames[0], frames[1], frames[2]]), [at(0, 60, grid_hz(900.0), 6480)])
    return {k: (np.ascontiguousarray(v[0], np.float32), np.array(v[1], ITEM_DTYPE).reshape(-1)) for k, v in out.items()}


def offsets_table(name):
    """the per-frame offsets the host builds of a case's items: offsets[f] = the number of items on frames before f"""
    audio, items = kernel_cases()[name]
    return [int((items["frame"] < f).sum()) for f in range(audio.shape[0])]


@functools.lru_cache(maxsize=None)
def kernel_fits(name, seed=SEED):
    """the restatement on a kernel case: (sub SUB_DTYPE[n], residual float32 [n_frames][N], fits [n]), read-only"""
    audio, items = kernel_cases()[name]
    if name == "reversed":
        # a fit reads the original frame alone: the 24 fits are those of "crowded", frame 3, made once; the order they are applied in is what differs
        csub, cres, cfits = kernel_fits("crowded", seed)
        sub, fits = csub[1:25][::-1].copy(), cfits[1:25][::-1]
        res = S.apply(audio[0], fits)[None, :]
        sub.setflags(write=False)
        res.setflags(write=False)
        return sub, res, fits
    sub = np.zeros(len(items), S.SUB_DTYPE)
    res = np.zeros_like(audio)
    fits = [None] * len(items)
    for f in range(audio.shape[0]):
        idx = [i for i in range(len(items)) if items["frame"][i] == f]
        recs, res[f], ft = S.subtract(audio[f], [(tones(items["bits"][i], seed), items["freq_hz"][i], items["dt_s"][i]) for i in idx])
        sub[idx] = recs
        for i, x in zip(idx, ft):
            fits[i] = x
    sub.setflags(write=False)
    res.setflags(write=False)
    return sub, res, fits


def kernel_reference(name, seed=SEED):
    return kernel_fits(name, seed)[:2]
