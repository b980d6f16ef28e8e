"""Further inputs of the FT8 subtractor's flat call (tests/test_subtract_edge_inputs.py proves on the CPU what each one contains;
tests/test_gpu_ft8_subtract_kernel.py runs them on the device): starts off the 40 ms grid, so that the window's alignment remainder w0 mod 4 of
modules/ft8sub.hip's sub_tile_pass is 1, 2 and 3 as well as 0; items at the limits the host accepts; a table of offsets with runs of equal entries
and one frame with 24 items; that frame with its items in reverse order.  Built with tests/ft8_subtract_cases.py's helpers; every reference is
computed once and shared."""
import functools

import numpy as np

import ft8_subtract_ref as S
from ft8_subtract_cases import ITEM_DTYPE, SEED, item, noise, tones, tx, word  # noqa: F401  (word: for the tests)

N = S.N
FS = 12000.0
TONE_HZ = 6.25
NAMES = ("offgrid", "limits", "crowded", "reversed", "trailing")


def at(frame, k, freq_hz, samples):
    """an item whose dt_s is `samples` / 12000: the start the kernel derives is samples + 6000 - 480"""
    return item(frame, k, freq_hz, np.float32(samples / FS))


def sent(k, f_hz, samples, amp, phase0=0.0):
    """the transmission of word k whose first sample is 6000 + `samples`"""
    return tx(k, f_hz, samples / FS, amp, phase0)


# offgrid: (word, true frequency, the item's dt_s in samples, true first sample minus the centre of the item's time search, amplitude).  The
# window of tile 0 starts at w0 = samples + 5280, so w0 mod 4 is samples mod 4: 0, 1, 2, 3.  The time grid has 8 samples: the four starts are 0, +43,
# -21 and +5 samples from the centre, and the restatement's winners are 0, 6, -2 and 1 steps.
OFFGRID = ((20, 700.3, 1200, 0, 600.0), (21, 1333.3, -3719, 43, 500.0), (22, 1999.1, 6002, -21, 700.0), (23, 2600.7, 2403, 5, 400.0))
# limits: the items in front of the real transmission (word, frequency, dt_s): both ends of dt_s; a window whose earliest offset leaves the last 50
# samples of the frame to the signal's first block; one whose latest offset leaves the frame's first 50 samples to the signal's last block; both
# ends of freq_hz
SLIVER_END = (N - 50 + S.TAU_MAX - 6000 + S.CAND_STEP) / FS
SLIVER_START = (50 - S.NW - S.TAU_MAX - 6000 + S.CAND_STEP) / FS
LIMITS = ((31, 1000.0, 30.0), (32, 1000.0, -30.0), (33, 1500.0, SLIVER_END), (34, 1500.0, SLIVER_START), (35, 0.0, 0.52), (36, 6000.0, 0.52))
LIMITS_TX = (30, 1750.0, 0.3, 800.0)
# crowded, frame 3: twelve transmissions (word, frequency, first sample - 6000, amplitude); the first four are pairwise within one tone spacing
# (6.25 Hz) and overlap in time
CROWD = ((40, 1000.0, 1200, 500.0), (41, 1002.0, 1800, 450.0), (42, 1004.0, 600, 400.0), (43, 1005.5, 2400, 550.0),
         (44, 400.0, -2400, 300.0), (45, 650.0, 0, 350.0), (46, 1300.0, 4801, 600.0), (47, 1600.0, 3602, 250.0),
         (48, 1900.0, 7203, 700.0), (49, 2200.0, -1199, 320.0), (50, 2500.0, 9600, 380.0), (51, 2800.0, 12001, 420.0))
CROWD_COUNTS = {0: 1, 3: 24, 7: 2}
CROWD_FRAMES = 8


def grid_hz(f_hz):
    return 3.125 * round(f_hz / 3.125)


def _crowd_frame():
    return sum(sent(k, f, s, a, 0.37 * i) for i, (k, f, s, a) in enumerate(CROWD)) + noise(43, 120.0)


def _crowd_items(frame):
    """each of the twelve named twice: as a candidate would carry it, then 1 Hz and 3 samples away"""
    first = [at(frame, k, grid_hz(f), s + S.CAND_STEP) for k, f, s, a in CROWD]
    second = [at(frame, k, grid_hz(f) + 1.0, s + S.CAND_STEP + 3) for k, f, s, a in CROWD]
    return first + second


@functools.lru_cache(maxsize=None)
def kernel_cases():
    """name -> (audio float32 [n_frames][N], items ITEM_DTYPE[n])"""
    out = {}
    a = sum(sent(k, f, s - S.CAND_STEP + d, amp, 0.9 * i) for i, (k, f, s, d, amp) in enumerate(OFFGRID)) + noise(31, 150.0)
    out["offgrid"] = (a[None, :], [at(0, k, grid_hz(f), s) for k, f, s, d, amp in OFFGRID])
    k, f, dt, amp = LIMITS_TX
    a = tx(k, f, dt, amp, 0.4) + noise(32, 200.0)
    out["limits"] = (a[None, :], [item(0, w, fq, np.float32(d)) for w, fq, d in LIMITS] + [at(0, k, grid_hz(f), round(dt * FS) + S.CAND_STEP)])
    frames = [noise(40 + i, 100.0 + 10.0 * i) for i in range(CROWD_FRAMES)]
    frames[0] = frames[0] + sent(60, 900.0, 480, 500.0)
    frames[3] = _crowd_frame()
    frames[7] = frames[7] + sent(61, 1200.0, -960, 400.0) + sent(62, 2000.0, 2405, 600.0, 1.0)
    out["crowded"] = (np.stack(frames), [at(0, 60, grid_hz(900.0), 480 + S.CAND_STEP)] + _crowd_items(3)
                      + [at(7, 61, grid_hz(1200.0), -960 + S.CAND_STEP), at(7, 62, grid_hz(2000.0), 2405 + S.CAND_STEP)])
    out["reversed"] = (frames[3][None, :], _crowd_items(0)[::-1])
    # three frames, the last two without an item: the tail of the offsets table is filled on more than one frame
    out["trailing"] = (np.stack([frames[0], frames[1], frames[2]]), [at(0, 60, grid_hz(900.0), 480 + S.CAND_STEP)])
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
