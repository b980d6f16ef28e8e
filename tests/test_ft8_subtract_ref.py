"""CPU: the FT8 subtractor's restatement (tests/ft8_subtract_ref.py) and its inputs -- the committed tables, the header's exports, and what the
statement does on frames made by the independent float64 GFSK synthesiser (tests/ft8_gfsk.py): refinement, an absent word, signals cut by the
frame's edges, overlapping signals, one word twice; the removal depth as a measured property against a float64 implementation."""
import importlib.util
import os
import re

import numpy as np
import pytest

import ft8_subtract_cases as SC
import ft8_subtract_quality as Q
import ft8_subtract_ref as S

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_tables_regenerate_to_the_committed_literals():
    spec = importlib.util.spec_from_file_location("gen_ft8sub_tables", os.path.join(ROOT, "scripts", "gen_ft8sub_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.render() == open(S.TABLES_INC).read()
    t = S.parse_tables()
    assert t["FT8SUB_CP"].size == 3 * 1920 and t["FT8SUB_CPT"].size == 3 and t["FT8SUB_COSQ"].size == 1025 and t["FT8SUB_WIN"].size == 97
    # a whole symbol of one tone unit turns the phase once (6.25 Hz over 160 ms), up to the rounding of 5760 increments
    assert abs(int(t["FT8SUB_CPT"].astype(np.int64).sum()) - (1 << 32)) < 5760
    # no kernel source of the module, and not the restatement, calls a sine or cosine
    src = open(os.path.join(ROOT, "cwsl_digi_amd", "csrc", "modules", "ft8sub.hip")).read()
    assert not re.search(r"\b(__)?(sin|cos|sincos)f?\s*\(", src)
    assert not re.search(r"np\.(cos|sin|exp)\b", open(os.path.join(ROOT, "tests", "ft8_subtract_ref.py")).read().split('"""', 2)[2])


def test_header_declares_the_exports_and_abi_5():
    h = open(os.path.join(ROOT, "include", "cwsl_gpu.h")).read()
    assert re.search(r"#define CWSLG_ABI_VERSION 5\b", h)
    for name in ("cwslg_subtract_ft8", "cwslg_fetch_ft8_residual", "cwslg_ft8_residual_device_ptr", "cwslg_ft8_subtract_flat"):
        assert re.search(r"^int\s+%s\(" % name, h, re.M), name
    assert "} cwslg_subtract_report;" in h and "PARITY UNPINNED" in h.split("/* FT8 signal subtraction", 1)[1][:200]
    # the second pass, not the subtraction, is what stays out of scope
    assert not re.search(r"[^4(] signal subtraction,", h)
    from cwsl_digi_amd import api
    assert api.SUBTRACT_REPORT_DTYPE == S.SUB_DTYPE and api.FT8_SUB_ITEM_DTYPE == SC.ITEM_DTYPE
    assert {"cwslg_subtract_ft8", "cwslg_fetch_ft8_residual", "cwslg_ft8_residual_device_ptr", "cwslg_ft8_subtract_flat"} <= set(api.ABI_SYMBOLS)


# The grids of the statement: the time search steps by 8 samples, the frequency search by 11185 * 12000 / 2^32 Hz.  A noise-free transmission is
# found at the grid point nearest to the truth or at a neighbour of it -- the metric is symmetric about the truth and falls off on both sides --
# so the refined values lie within ONE step of the truth.  The condition follows from the grid, not from a measurement.
TIME_STEP_S = 8 / 12000.0
FREQ_STEP_HZ = 11185 * 12000.0 / 4294967296.0


@pytest.mark.parametrize("k,f,dt", [(0, 1234.56, 0.1237), (1, 801.3, -0.31), (2, 1500.9, 1.013), (3, 2001.5, 0.2199), (4, 651.6, 1.58)])
def test_noise_free_transmissions_are_refined_to_the_grid(k, f, dt):
    assert (S.TIME_STEP_S, S.FREQ_STEP_HZ) == (TIME_STEP_S, FREQ_STEP_HZ)
    fg, dtg = SC.grid(f, dt)
    assert abs(fg - f) <= 1.5625 and abs(dtg - 0.04 - dt) <= 0.02 + 1e-9    # the candidate: half a bin, half a plane step (dt_s one step late)
    x = SC.tx(k, f, dt, 1000.0, 0.4 + k).astype(np.float32)
    rec, _ = S.fit(x, SC.tones(SC.word(k)), fg, dtg)
    assert abs(float(rec["f_hz"]) - f) <= FREQ_STEP_HZ, rec
    assert abs(float(rec["dt_s"]) - dt) <= TIME_STEP_S, rec
    assert rec["n_inside"] == S.NW and rec["p_after"] < 0.01 * rec["p_before"]


def test_a_word_the_frame_does_not_contain():
    """Noise alone.  The track averages the block sums under a Hann window of 97 blocks, whose equivalent noise width is 65 blocks ((sum w)^2 /
    sum w^2 = 49^2 / 36.75): the fit can take out 1/65 of the footprint's noise energy, times what the two searches gain by choosing among 61
    and 105 correlated points.  Stated relation, with a factor 4 for that choice: removed <= before / 16 and after >= before (1 - 1/8)."""
    x = SC.noise(31, 500.0).astype(np.float32)
    rec, f = S.fit(x, SC.tones(SC.word(9)), 1400.0, 0.5)
    assert 0 <= rec["p_removed"] <= rec["p_before"] / 16, rec
    assert rec["p_after"] >= rec["p_before"] * (1 - 1 / 8), rec
    res = S.apply(x, [f])
    assert S.footprint_power(res, f) >= S.footprint_power(x, f) * (1 - 1 / 8)
    e0, e1 = float(np.sum(x.astype(np.float64) ** 2)), float(np.sum(res.astype(np.float64) ** 2))
    assert abs(e1 - e0) <= e0 / 16


@pytest.mark.parametrize("dt,side", [(-1.2, "start"), (2.43, "end")])
def test_a_signal_cut_by_a_frame_edge(dt, side):
    k, f = 5, 1100.4
    x = SC.tx(k, f, dt, 800.0, 1.1).astype(np.float32)
    fg, dtg = SC.grid(f, dt)
    rec, ft = S.fit(x, SC.tones(SC.word(k)), fg, dtg)
    start = ft["start"]
    assert (start < 0) if side == "start" else (start + S.NW > S.N)
    assert rec["n_inside"] == min(start + S.NW, S.N) - max(start, 0) < S.NW
    res = S.apply(x, [ft])
    # the edge is not pulled down: the track is normalised by the samples under the window, so the first / last second goes like the middle
    seg = slice(0, 12000) if side == "start" else slice(S.N - 12000, S.N)
    assert np.sum(res[seg].astype(np.float64) ** 2) < 1e-3 * np.sum(x[seg].astype(np.float64) ** 2)
    assert np.sum(res.astype(np.float64) ** 2) < 1e-3 * np.sum(x.astype(np.float64) ** 2)


def test_two_signals_overlapping_in_time_and_frequency():
    """40 Hz apart (their 50 Hz-wide tone sets interleave), 0.3 s apart, equal strength.  Each is fitted from the original frame with the other in
    it: the other's tones pass through the 200 Hz-wide block sums but beat against this one's at 6.25 Hz multiples, which the 0.48 s window averages
    down.  Not a joint fit, so the depth is that of a single signal in strong interference: the residual holds less than a tenth of the energy."""
    t2, t3 = SC.tones(SC.word(2)), SC.tones(SC.word(3))
    x = (SC.tx(2, 1500.9, 1.013, 700.0, 1.0) + SC.tx(3, 1540.3, 0.71, 700.0, 2.0)).astype(np.float32)
    recs, res, fits = S.subtract(x, [(t2, *SC.grid(1500.9, 1.013)), (t3, *SC.grid(1540.3, 0.71))])
    # (no grid argument bounds the refinement here: each search sees the other signal; both land within a tenth of a hertz)
    assert abs(float(recs["f_hz"][0]) - 1500.9) <= 0.1 and abs(float(recs["f_hz"][1]) - 1540.3) <= 0.1, recs
    assert np.sum(res.astype(np.float64) ** 2) < 0.1 * np.sum(x.astype(np.float64) ** 2)
    # emission order is the order of subtraction: the other order gives another float32 sum
    _, other, _ = S.subtract(x, [(t3, *SC.grid(1540.3, 0.71)), (t2, *SC.grid(1500.9, 1.013))])
    assert np.allclose(other, res, atol=1e-2) and np.sum(other.astype(np.float64) ** 2) < 0.1 * np.sum(x.astype(np.float64) ** 2)


def test_the_same_word_twice_at_different_frequencies():
    t = SC.tones(SC.word(2))
    x = (SC.tx(2, 900.4, 0.33, 600.0, 0.2) + SC.tx(2, 2450.4, 0.52, 300.0, 0.3)).astype(np.float32)
    recs, res, fits = S.subtract(x, [(t, *SC.grid(900.4, 0.33)), (t, *SC.grid(2450.4, 0.52))])
    assert abs(float(recs["f_hz"][0]) - 900.4) <= FREQ_STEP_HZ and abs(float(recs["f_hz"][1]) - 2450.4) <= FREQ_STEP_HZ
    assert (recs["p_after"] < 0.01 * recs["p_before"]).all(), recs
    assert np.sum(res.astype(np.float64) ** 2) < 1e-2 * np.sum(x.astype(np.float64) ** 2)


# Removal depth, float32 restatement against the float64 implementation (tests/ft8_subtract_quality.py; profiles/ft8_subtract_quality.json holds
# the figures).  Measured over the twelve cases: db32 - db64 between -0.001 and +0.263 dB; the +0.26 is at the -56 dB floor of the on-grid
# noise-free case, where the 12-bit phase table (-67 dB) and float32 sums begin to count; everywhere above -50 dB the two agree to 0.01 dB.
# MARGIN: 1 dB, four times the largest difference measured -- wide enough for another libm's last bit in the synthesiser, far too narrow for a
# wrong table or a lost bit of phase to pass (a 10-bit table would cost 10 dB at the floor).
MARGIN_DB = 1.0


def test_removal_depth_float32_against_float64():
    rows = Q.measure()
    assert len(rows) == 12
    for r in rows:
        print("word %d f %.2f dt %.4f sigma %6.0f: float32 %.2f dB, float64 %.2f dB" % (r["word"], r["f_hz"], r["dt_s"], r["sigma"], r["db32"], r["db64"]))
    worst = max(r["db32"] - r["db64"] for r in rows)
    assert worst <= MARGIN_DB, worst
    assert all(r["db32"] < -30 for r in rows if r["sigma"] == 0)        # (the cases do remove something: noise-free, better than 30 dB)
