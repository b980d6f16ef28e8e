"""CPU: the two finalise references of tests/fused_finalise_check.py (the oracle's prepare_audio + to_int16, and plain numpy float32) pinned against
each other bit for bit where a finalise goes wrong -- rounding ties, both sides of -0.5, full scale, the empty frame, n_valid at the frame's edges --
and the helper's own plumbing (the workgroup split it labels failures with, the bounded job queue)."""
import os
import re
import threading

import numpy as np
import pytest

from fused_finalise_check import SlotJobs, cpu_finalise, numpy_finalise, spectra_jper

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = ["FT8", "FT4", "WSPR", "FST4W-120"]


def _same(a, nv, mode):
    i_c, f_c = cpu_finalise(a, nv, mode)
    i_n, f_n = numpy_finalise(a, nv, mode)
    assert f_c.view(np.uint32) == f_n.view(np.uint32), (mode, nv, f_c, f_n)
    assert i_c.dtype == i_n.dtype == np.int16 and np.array_equal(i_c, i_n), (mode, nv, np.nonzero(i_c != i_n)[0][:8])
    assert not i_c[nv:].any()
    return i_c, f_c


def _factor(peak, mode):
    f = np.float32(32767.0) / (np.float32(peak) + np.float32(1.0))
    return np.float32(f * np.float32(0.20 if mode == "WSPR" else 0.90))


@pytest.mark.parametrize("mode", MODES)
def test_random_frame_and_n_valid_edges(oracle, mode):
    n = oracle.frame_len(mode)
    rng = np.random.default_rng(7)
    a = (rng.standard_normal(n) * 1500.0).astype(np.float32)
    a[n // 3] = np.float32(-9000.25)                                           # the peak is a negative sample
    for nv in (0, 4, 12, n):
        i16, f = _same(a, nv, mode)
        peak = np.abs(a[:nv]).max() if nv else 0.0
        assert f.view(np.uint32) == _factor(peak, mode).view(np.uint32)
        assert i16[:nv].any() == (nv > 0)
    # what lies beyond n_valid does not count, not even for the peak
    b = a.copy(); b[12:] = 1e9
    assert np.array_equal(_same(b, 12, mode)[0], _same(a, 12, mode)[0])


@pytest.mark.parametrize("mode", ["FT8", "WSPR"])
def test_all_zero_frame(oracle, mode):
    n = oracle.frame_len(mode)
    for nv in (0, n):
        i16, f = _same(np.zeros(n, np.float32), nv, mode)
        assert f == np.float32(32767.0) * np.float32(0.20 if mode == "WSPR" else 0.90) and not i16.any()


@pytest.mark.parametrize("mode", ["FT8", "WSPR"])
@pytest.mark.parametrize("peak", [1e-3, 1.0, 40.0, 32767.0, 2.0 ** 24, 1e30])
def test_ties_and_both_sides_of_minus_half(oracle, mode, peak):
    """Samples whose scaled value x * factor lies on, just below and just above k + 0.5 and k - 0.5 for small and large k of either sign: the
    boundaries of (int16)(x * factor + 0.5f) are 0.5, 1.5, ... and -1.5, -2.5, ...; -0.5 is none, because truncation goes toward zero, so samples on
    both sides of it give 0.  Next to them a full-scale sample of either sign."""
    f = _factor(peak, mode)
    top = int(np.float32(peak) * f)
    ks = sorted({k for k in (0, 1, 2, 3, 100, 1000, 12345, top - 1, top) if 0 <= k <= top})
    xs = [np.float32(peak), np.float32(-peak)]
    for k in ks:
        for t in (k + 0.5, k - 0.5, -(k + 0.5), -(k - 0.5), float(k), -float(k), -0.49, -0.51, -1.49, -1.51):
            x = np.float32(np.float32(t) / f)
            if abs(x) > np.float32(peak):
                continue
            lo, hi = np.nextafter(x, np.float32(-np.inf)), np.nextafter(x, np.float32(np.inf))
            xs += [x, lo, hi, np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))]
    a = np.array([x for x in xs if abs(x) <= np.float32(peak)], np.float32)
    i16, fac = _same(a, len(a), mode)
    assert fac.view(np.uint32) == f.view(np.uint32)
    # the rule itself, sample by sample, in Python floats rounded to float32 at each step
    for x, q in zip(a, i16):
        s = np.float32(x * f); b = np.float32(s + np.float32(0.5))
        assert int(q) == int(b), (x, s, b, q)                                      # int(): truncation toward zero
    assert i16[0] in (top, top + 1) and i16.min() >= -top - 1                     # full scale stays inside int16: |x * factor| <= 32767 * scale


def test_known_values(oracle):
    # peak 40: factor = 32767 / 41 * 0.9; the frame of tests/test_oracle_framing.py::test_prepare_audio_rules
    a = np.array([0, 10, -40, 5, 0, 0], np.float32)
    i16, f = _same(a, 6, "FT8")
    assert f == np.float32(np.float32(32767.0) / np.float32(41.0)) * np.float32(0.90)
    assert list(i16) == [0, 7193, -28770, 3596, 0, 0]      # 7192.756 + 0.5 -> 7193; -28771.023 + 0.5 -> -28770 (toward zero); 3596.378 + 0.5 -> 3596


def test_jper_restatement_matches_the_header():
    src = open(os.path.join(ROOT, "cwsl_digi_amd", "csrc", "sync_kernels.hpp")).read()
    m = re.search(r"inline int spectra_jper\(int nsteps, size_t channels\)\s*\{(.*?)\n\}", src, re.S)
    assert m, "spectra_jper not found"
    body = m.group(1)
    assert re.search(r"for \(int jper : \{62, 31\}\)", body) and ">= 3072) return jper" in body and "return 12;" in body
    assert "(nsteps + jper - 1) / jper" in body
    assert [spectra_jper(n) for n in (1, 8, 255, 256, 300, 511, 512, 600, 4096)] == [12, 12, 12, 31, 31, 31, 62, 62, 62]


def test_slot_jobs_queue_is_bounded_and_reports_failures():
    live, peak, lock = [0], [0], threading.Lock()
    gate = threading.Event()

    def job():
        with lock:
            live[0] += 1; peak[0] = max(peak[0], live[0])
        gate.wait(0.01)
        with lock:
            live[0] -= 1

    with SlotJobs(depth=8) as q:
        assert q.pool._max_workers == min(16, len(os.sched_getaffinity(0)))
        for _ in range(100):
            q.submit(job)
            assert len(q.pending) < 8
        q.drain()
        assert q.done == 100 and peak[0] <= 8

    def bad():
        raise AssertionError("slot 3: wrong")

    with pytest.raises(AssertionError, match="slot 3"):
        with SlotJobs(depth=4) as q:
            q.submit(job); q.submit(bad); q.submit(job)
