"""CPU: the recipes of tests/longsync_cases.py do what tests/test_gpu_longsync_edges.py assumes, shown on the restatement alone.

The IQ of both receivers goes through the oracle's own chain (oracle.Channel(mode, 48000, 2048, dial): boundary, push_many, boundary -- the
frames that the library's exact mode reproduces bit for bit), then through oracle.wspr_search / oracle.fst4w_candidates.  Conditions:
  1  the minsync 0.1 window (1400..1607) reaches exactly 100 records on at least one channel;
  2  the all-zero frame gives exactly one FST4W record, (bin == ia, snr NaN), and at least 10 WSPR candidates;
  3  the edge carriers are strict maxima of smspec in bins +150 / -151 (W_carriers) and -150 / +151 (W_tx); the lists hold exactly the
     maxima of bins -150 .. +150, one of them the edge carrier's, and nothing from beyond;
  4  every other list of the default window is non-empty;
  5  the npts < 1 window gives no record on any channel, the npts 2 and 3 windows none or few (at most one per bin of ia .. ib);
  6  the bounds of the library's window check, restated in float32 numpy (longsync_cases.fst4w_window), accept every window of the walk
     and 1400..1607 (nband 24936: exactly 200 per residue) and refuse 1400..1608 (nband 25111).
A recipe that misses its condition is changed (seed, amplitude), never the condition.

Cost: 11 frames through the oracle's chain and 41 searches, about 15 s on one core."""
import numpy as np
import pytest

import longsync_cases as L


@pytest.fixture(scope="module")
def frames(oracle):
    iq_a, iq_b = L.receiver_a_iq(oracle), L.receiver_b_iq()
    fr = {n: L.oracle_frame(oracle, n, iq_a) for n, _, _ in L.A_CHANNELS}
    fr.update({n: L.oracle_frame(oracle, n, iq_b) for n, _, _ in L.B_CHANNELS})
    return fr


def test_frames_are_what_the_recipes_say(frames):
    assert not frames["W_zero"].any() and not frames["F_zero"].any()
    for n, _, _ in L.A_CHANNELS:
        fr = frames[n]
        assert len(fr) >= 1440000 and fr[:L.N // 4].any() and not fr[L.N // 4:].any()      # 30 s of audio, then the zero tail


def test_cap_is_reached(oracle, frames):
    nfa, nfb, minsync = L.WALK[5]
    n = [len(oracle.fst4w_candidates(frames[c], nfa, nfb, minsync)) for c in L.A_FST]
    assert max(n) == 100, n


def test_zero_frame(oracle, frames):
    nfa, nfb, minsync = L.DEFAULT_WINDOW
    ref = oracle.fst4w_candidates(frames["F_zero"], nfa, nfb, minsync)
    ia = L.fst4w_window(nfa, nfb)["ina"]
    assert len(ref) == 1 and ref[0][2] == ia == 1913 and np.isnan(ref[0][1]) and abs(ref[0][0] - 1399.7561) < 1e-3
    cands, arr = oracle.wspr_search(frames["W_zero"], want_arrays=True)
    assert len(cands) >= 10 and len(L.smspec_peaks(arr["smspec"])) > len(cands)          # a nearly flat spectrum: peaks on both sides of +-110 Hz


def test_edge_carriers(oracle, frames):
    for name, kept, dropped in (("W_carriers", 150, -151), ("W_tx", -150, 151)):
        cands, arr = oracle.wspr_search(frames[name], want_arrays=True)
        peaks = L.smspec_peaks(arr["smspec"])
        assert kept in peaks and dropped in peaks, (name, peaks)
        assert len(cands) == len([p for p in peaks if abs(p) <= 150]) < len(peaks), (name, len(cands), peaks)
        f = np.array([c[0] for c in cands])
        # the coarse search moves a peak by up to two bins; the carrier is one of the two strongest entries
        assert np.abs(f[:2] - kept * L.DFW).min() <= 2 * L.DFW + 1e-4, (name, cands[:2])
        assert np.abs(f).max() <= 152 * L.DFW + 1e-4
        # the dropped carrier owns smspec's bins 148 .. 154 of its side: the nearest peak that could be kept is 147, +2 bins of the coarse search
        assert (f * np.sign(dropped)).max() <= 149 * L.DFW + 1e-4, (name, sorted(f))


def test_default_window_lists_are_non_empty(oracle, frames):
    nfa, nfb, minsync = L.DEFAULT_WINDOW
    for c in L.A_FST:
        assert len(oracle.fst4w_candidates(frames[c], nfa, nfb, minsync)) >= 1, c
    for c in L.A_WSPR:
        assert len(oracle.wspr_search(frames[c])) >= 1, c


def test_degenerate_windows(oracle, frames):
    for k, want_npts in ((6, 3), (7, 2), (8, None)):
        nfa, nfb, minsync = L.WALK[k]
        w = L.fst4w_window(nfa, nfb)
        n = [len(oracle.fst4w_candidates(frames[c], nfa, nfb, minsync)) for c in L.A_FST + ["F_zero"]]
        if want_npts is None:
            assert w["npts"] < 1 and n == [0] * len(n), (k, w, n)
        else:
            assert w["npts"] == want_npts and max(n) <= w["inb"] - w["ina"] + 1, (k, w, n)


def test_window_limits_restated():
    for nfa, nfb, _ in L.WALK:
        assert L.fst4w_window(nfa, nfb) is not None, (nfa, nfb)
    w = L.fst4w_window(1400, 1607)
    assert w["nband"] == 24936 and (w["nband"] + 124) // 125 == 200
    assert L.fst4w_window(*L.REJECTED_WINDOW) is None and L.fst4w_window(*L.REJECTED_WINDOW, table_limits=False)["nband"] == 25111
    # the clamps: 50 Hz reads as 100 Hz, 4900 Hz as 4800 Hz
    assert L.fst4w_window(50, 250)["ina"] == L.fst4w_window(100, 250)["ina"] == 137
    assert L.fst4w_window(4700, 4900)["inb"] == L.fst4w_window(4700, 4800)["inb"] == 6560
    # the second table limit, jlo > 125, cannot be reached: the 100 Hz clamp keeps jlo at 11986
    assert min(L.fst4w_window(a, 300)["jlo"] for a in (-1000, 0, 50, 100)) == 11986
    # other refusals: an inverted window, and more than 1024 comb bins
    assert L.fst4w_window(1600, 1400) is None and L.fst4w_window(100, 4800) is None
