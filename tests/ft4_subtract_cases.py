"""Inputs of the FT4 subtractor's tests (tests/test_ft4_subtract_ref.py on the CPU, tests/test_gpu_ft4_subtract_kernel.py on the device): frames
made with the float64 GFSK synthesiser (tests/ft4_gfsk.py) and words re-encoded under the code of a seed through the FT4 tone mapping
(tests/ft4_decode_reports_ref.py), as everywhere in the chain's tests.  Every reference (tests/ft4_subtract_ref.py) is computed once and shared."""
import functools

import numpy as np

import ft4_decode_reports_ref as R4
import ft4_gfsk as G
import ft4_subtract_ref as S
import report_kernel_cases as K

SEED = K.SEED
N = S.N
ITEM_DTYPE = np.dtype([("frame", np.int32), ("bits", np.uint8, 12), ("freq_hz", np.float32), ("dt_s", np.float32)])
BASEBAND_HZ = 12000.0 / 18.0                       # the 666.67 Hz baseband in which a record's ibest is found


def word(k):
    """the k-th 91-bit test word, as bits[12]"""
    rng = np.random.default_rng(7400 + k)
    b = rng.integers(0, 256, 12, dtype=np.uint8)
    b[11] &= 0xE0
    return b


def tones(bits12, seed=SEED):
    return R4.tones(K.encoder(seed), bits12)


def noise(seed, sigma):
    return sigma * np.random.default_rng(seed).standard_normal(N)


def tx(k, f_hz, dt_s, amp=1.0, phase0=0.0):
    return G.synth(tones(word(k)), f_hz, dt_s, amp, phase0)


def item(frame, k, freq_hz, dt_s):
    it = np.zeros((), ITEM_DTYPE)
    it["frame"], it["bits"], it["freq_hz"], it["dt_s"] = frame, word(k), freq_hz, dt_s
    return it


def grid(f_hz, dt_s):
    """the (f1_hz, dt_s) a sync record of the chain would carry for a transmission: the refinement's 1 Hz frequency grid, and the start on the
    666.67 Hz baseband's sample grid (dt_s = ibest / 666.67 - 0.5 names the first sample itself: no offset)"""
    return float(round(f_hz)), round((dt_s + 0.5) * BASEBAND_HZ) / BASEBAND_HZ - 0.5


@functools.lru_cache(maxsize=None)
def kernel_cases():
    """name -> (audio float32 [n_frames][N], items ITEM_DTYPE[n]): the shapes the kernels can go wrong at -- one item; an empty frame, one item,
    four in emission order (two of them overlapping in time and frequency, one word twice at two frequencies); a signal that starts before sample
    0 and one cut by the frame's end (a start of 1.2 s ends 1152 samples past 72576); an all-zero frame; no item at all."""
    out = {}
    a = tx(0, 1234.56, 0.1237, 900.0, 0.7) + noise(11, 300.0)
    out["one"] = (a[None, :], [item(0, 0, *grid(1234.56, 0.1237))])
    f1 = tx(1, 801.3, -0.31, 500.0) + noise(12, 100.0)
    f2 = (tx(2, 1500.9, 0.413, 700.0, 1.0) + tx(3, 1521.2, 0.33, 250.0, 2.0) + tx(4, 2100.0, 0.2, 400.0) + tx(2, 2450.4, -0.08, 300.0, 0.3) + noise(13, 150.0))
    out["zero_one_four"] = (np.stack([noise(14, 200.0), f1, f2]),
                            [item(1, 1, *grid(801.3, -0.31)), item(2, 2, *grid(1500.9, 0.413)), item(2, 3, *grid(1521.2, 0.33)), item(2, 4, *grid(2100.0, 0.2)),
                             item(2, 2, *grid(2450.4, -0.08))])
    assert int(round((0.7 + 0.5) * 12000)) + S.NW - N == 1152
    e = tx(5, 700.0, -0.62, 600.0) + tx(6, 1900.0, 0.7, 600.0) + noise(15, 50.0)
    out["edges"] = (e[None, :], [item(0, 5, *grid(700.0, -0.62)), item(0, 6, *grid(1900.0, 0.7))])
    out["silence"] = (np.zeros((1, N)), [item(0, 7, 1000.0, 0.0)])
    out["no_items"] = (np.stack([noise(16, 10.0), noise(17, 20.0)]), [])
    return {k: (np.ascontiguousarray(v[0], np.float32), np.array(v[1], ITEM_DTYPE).reshape(-1)) for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def kernel_reference(name, seed=SEED):
    """the restatement on a kernel case: (sub SUB_DTYPE[n], residual float32 [n_frames][N]), read-only"""
    audio, items = kernel_cases()[name]
    sub = np.zeros(len(items), S.SUB_DTYPE)
    res = np.zeros_like(audio)
    for f in range(audio.shape[0]):
        idx = [i for i in range(len(items)) if items["frame"][i] == f]
        recs, res[f], _ = S.subtract(audio[f], [(tones(items["bits"][i], seed), items["freq_hz"][i], items["dt_s"][i]) for i in idx])
        sub[idx] = recs
    sub.setflags(write=False)
    res.setflags(write=False)
    return sub, res
