"""CPU: the FT4 subtractor's restatement (tests/ft4_subtract_ref.py) and its inputs -- the committed tables, the header's exports, and what the
statement does on frames made by the independent float64 GFSK synthesiser (tests/ft4_gfsk.py): the waveform itself, refinement, signals cut by the
frame's edges, an all-zero frame, two decodes in emission order; the removal depth as a measured property against a float64 implementation."""
import importlib.util
import math
import os
import re

import numpy as np
import pytest

import ft4_gfsk as G
import ft4_subtract_cases as SC
import ft4_subtract_quality as Q
import ft4_subtract_ref as S
import ft8_subtract_ref as S8

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def test_tables_regenerate_to_the_committed_literals():
    spec = importlib.util.spec_from_file_location("gen_ft4sub_tables", os.path.join(ROOT, "scripts", "gen_ft4sub_tables.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert gen.render() == open(S.TABLES_INC).read()
    t = S.parse_tables()
    assert t["FT4SUB_CP"].size == 3 * 576 and t["FT4SUB_CPT"].size == 3 and t["FT4SUB_COSQ"].size == 1025 and t["FT4SUB_WIN"].size == 97
    # a whole symbol of one tone unit turns the phase once (20.8333 Hz over 48 ms), up to the rounding of 1728 increments
    assert abs(int(t["FT4SUB_CPT"].astype(np.int64).sum()) - (1 << 32)) < 1728
    # the cosine quarter and the window are the FT8 subtractor's, bit for bit
    assert t["FT4SUB_COSQ"].tobytes() == S8.COSQ.tobytes() and t["FT4SUB_WIN"].tobytes() == S8.WIN.tobytes()
    # no kernel source of the module, and not the restatement, calls a sine or cosine
    src = open(os.path.join(ROOT, "cwsl_digi_amd", "csrc", "modules", "ft4sub.hip")).read()
    assert not re.search(r"\b(__)?(sin|cos|sincos)f?\s*\(", src)
    assert not re.search(r"np\.(cos|sin|exp)\b", open(os.path.join(ROOT, "tests", "ft4_subtract_ref.py")).read().split('"""', 2)[2])


def test_header_declares_the_exports_and_abi_5():
    h = open(os.path.join(ROOT, "include", "cwsl_gpu.h")).read()
    assert re.search(r"#define CWSLG_ABI_VERSION 5\b", h)
    names = ("cwslg_subtract_ft4", "cwslg_fetch_ft4_residual", "cwslg_ft4_residual_device_ptr", "cwslg_ft4_subtract_flat")
    for name in names:
        assert re.search(r"^int\s+%s\(" % name, h, re.M), name
    assert "} cwslg_ft4_sub_item;" in h and re.search(r"#define CWSLG_FT4_FRAME_SAMPLES 72576\b", h)
    assert "PARITY UNPINNED" in h.split("/* FT4 signal subtraction", 1)[1][:200]
    assert "there is no FT4 subtraction" not in h
    from cwsl_digi_amd import api
    assert api.SUBTRACT_REPORT_DTYPE == S.SUB_DTYPE and api.FT4_SUB_ITEM_DTYPE == SC.ITEM_DTYPE and api.FT4_FRAME_SAMPLES == S.N
    assert set(names) <= set(api.ABI_SYMBOLS)
    shim = open(os.path.join(ROOT, "include", "cwsl_gpu_shim.hpp")).read()
    assert all(n in shim for n in ("subtractFt4", "ft4Residual", "ft4ResidualDevice", "ft4SubtractFlat"))
    # the layout header's constants are the restatement's
    lay = open(os.path.join(ROOT, "cwsl_digi_amd", "csrc", "ft4sub_layout.hpp")).read()
    for name, value in (("F4SUB_N", S.N), ("F4SUB_NSPS", S.NSPS), ("F4SUB_NSYM", S.NSYM), ("F4SUB_BLK", S.BLK), ("F4SUB_TAU_MAX", S.TAU_MAX), ("F4SUB_TAU_STEP", S.TAU_STEP),
                        ("F4SUB_DINC", S.DINC), ("F4SUB_KF", S.KF), ("F4SUB_CAND_OFFSET", S.CAND_OFFSET), ("F4SUB_HW", S.HW)):
        assert re.search(r"\b%s = %d\b" % (name, value), lay), name


# The restated waveform against the float64 synthesiser on the sample grid.  Both integrate the same per-sample increments; the restatement
# rounds each to an integer number of 2^-32 turns (the frequency's: half a unit; each of the three tone terms: half a unit times a tone of at
# most 3), which over 59328 samples adds up to at most 59328 * (0.5 + 3 * 1.5) units = 6.9e-5 turns, and reads a 4096-step table at the nearest
# step: half a step, 1 / 8192 turn.  |d cos| <= |d phase|, plus a float32 rounding of the table's value.
WAVE_BOUND = 2.0 * math.pi * (1.0 / 8192.0 + S.NW * (0.5 + 3 * 1.5) / 4294967296.0) + 2.0 ** -24


@pytest.mark.parametrize("k,f", [(0, 1234.56), (3, 2000.0), (5, 371.9)])
def test_waveform_against_the_float64_synthesiser(k, f):
    tones = SC.tones(SC.word(k))
    inc = S.inc_of(f)
    c, s = S.wave(tones, inc)
    ph = G.phase_track(tones, float(np.float32(f)), os=1)
    dc, ds = np.abs(c - np.cos(ph)).max(), np.abs(s - np.sin(ph)).max()
    print("largest difference: cos %.3e sin %.3e, bound %.3e" % (dc, ds, WAVE_BOUND))
    assert dc <= WAVE_BOUND and ds <= WAVE_BOUND
    # the bases are the waveform's own phase at the first sample of every symbol
    base = S.phase_bases(tones, inc)
    cb, sb = S.cos_sin(base)
    assert np.array_equal(cb, c[::S.NSPS]) and np.array_equal(sb, s[::S.NSPS])
    assert set(np.asarray(tones)[[0, 1, 2, 3]]) == {0, 1, 2, 3} and len(tones) == S.NSYM and max(tones) <= 3


def test_a_noise_free_transmission_on_both_grids_is_returned_as_it_is():
    """2000 Hz is on the records' 1 Hz grid, 0.202 s is baseband sample 468 (frame sample 8424): the record names the truth, and the fit stays"""
    k, f, dt = 3, 2000.0, 0.202
    assert SC.grid(f, dt) == (f, pytest.approx(dt, abs=1e-12))
    x = SC.tx(k, f, dt, 1000.0, 0.9).astype(np.float32)
    rec, ft = S.fit(x, SC.tones(SC.word(k)), *SC.grid(f, dt))
    assert ft["start"] == 8424 and (rec["df_steps"], rec["dt_steps"]) == (0, 0), rec
    # the searches stay on the record's grid point; the phase-slope step may move the increment by what the 4096-step table leaves of the track's
    # phase -- half a step, pi / 4096 rad, at either end of the 4.944 s signal: 2 (pi / 4096) / (2 pi 4.944) = 4.9e-5 Hz -- and f_hz is rounded to
    # float32, whose step at 2000 Hz is 1.22e-4 Hz
    assert abs(float(rec["f_hz"]) - 2000.0) <= 4.9e-5 + 1.22e-4 + 1e-9 and rec["dt_s"] == np.float32(8424 - 6000) / np.float32(12000.0), rec
    assert rec["n_inside"] == S.NW and rec["p_after"] < 0.001 * rec["p_before"] and abs(rec["p_removed"] / rec["p_before"] - 1) < 0.01


# The grids of the statement: the time search steps by 2 samples, the frequency search by 27962 * 12000 / 2^32 Hz.  A noise-free transmission is
# found at the grid point nearest to the truth or at a neighbour of it -- the metric is symmetric about the truth and falls off on both sides --
# so the refined values lie within ONE step of the truth.  The condition follows from the grid, not from a measurement.
TIME_STEP_S = 2 / 12000.0
FREQ_STEP_HZ = 27962 * 12000.0 / 4294967296.0


@pytest.mark.parametrize("k,f,dt", [(0, 1234.56, 0.1237), (1, 801.3, -0.31), (2, 1500.9, 0.413), (4, 651.6, 0.58)])
def test_noise_free_transmissions_are_refined_to_the_grid(k, f, dt):
    assert (S.TIME_STEP_S, S.FREQ_STEP_HZ) == (TIME_STEP_S, FREQ_STEP_HZ)
    fg, dtg = SC.grid(f, dt)
    assert abs(fg - f) <= 0.5 and abs(dtg - dt) <= 9 / 12000.0 + 1e-9      # the record: half a hertz, half a baseband sample
    x = SC.tx(k, f, dt, 1000.0, 0.4 + k).astype(np.float32)
    rec, _ = S.fit(x, SC.tones(SC.word(k)), fg, dtg)
    assert abs(float(rec["f_hz"]) - f) <= FREQ_STEP_HZ, rec
    assert abs(float(rec["dt_s"]) - dt) <= TIME_STEP_S, rec
    # p_after is a BLOCK-RATE figure: a real frame's image at -f passes the 18-sample block sums as a ripple the three-symbol window does not
    # follow, of relative size at most 1 / (18 |sin(2 pi f / 12000)|) -- the geometric sum over a block -- so its square bounds p_after / p_before,
    # beside the 0.5 % a start one sample off leaves at the symbol edges (2 of 576 samples).  The residual itself does not carry it (the depth
    # test below measures -54 dB)
    image = (1.0 / (S.BLK * abs(math.sin(2.0 * math.pi * f / 12000.0)))) ** 2
    print("p_after / p_before %.4f, bound %.4f" % (rec["p_after"] / rec["p_before"], image + 0.005))
    assert rec["n_inside"] == S.NW and rec["p_after"] < (image + 0.005) * rec["p_before"]


@pytest.mark.parametrize("dt,side", [(-0.62, "start"), (0.7, "end")])
def test_a_signal_cut_by_a_frame_edge(dt, side):
    k, f = 5, 1100.4
    x = SC.tx(k, f, dt, 800.0, 1.1).astype(np.float32)
    fg, dtg = SC.grid(f, dt)
    rec, ft = S.fit(x, SC.tones(SC.word(k)), fg, dtg)
    start = ft["start"]
    assert (start < 0) if side == "start" else (start + S.NW > S.N)
    assert rec["n_inside"] == min(start + S.NW, S.N) - max(start, 0) < S.NW
    assert abs(float(rec["f_hz"]) - f) <= FREQ_STEP_HZ and abs(float(rec["dt_s"]) - dt) <= TIME_STEP_S, rec
    res = S.apply(x, [ft])
    # the edge is not pulled down: the track is normalised by the samples under the window, so the first / last 0.3 s goes like the middle
    seg = slice(0, 3600) if side == "start" else slice(S.N - 3600, S.N)
    assert np.sum(res[seg].astype(np.float64) ** 2) < 1e-3 * np.sum(x[seg].astype(np.float64) ** 2)
    assert np.sum(res.astype(np.float64) ** 2) < 1e-3 * np.sum(x.astype(np.float64) ** 2)
    # outside the signal the frame keeps its bits
    a, b = max(start, 0), min(start + S.NW, S.N)
    assert res[:a].tobytes() == x[:a].tobytes() and res[b:].tobytes() == x[b:].tobytes()


def test_an_all_zero_frame():
    """Every sum is +0: the first maximum of every search is its first point (k = -26 twice, j = 0), the track and the figures are +0 and the
    residual is the frame's own zeros."""
    x = np.zeros(S.N, np.float32)
    recs, res, fits = S.subtract(x, [(SC.tones(SC.word(7)), 1000.0, 0.0)])
    r = recs[0]
    assert (r["df_steps"], r["dt_steps"]) == (-2 * S.KF, -(S.TAU_MAX // S.TAU_STEP)) and fits[0]["start"] == 6000 - S.TAU_MAX
    assert r["p_removed"] == 0 and r["p_before"] == 0 and r["p_after"] == 0 and r["n_inside"] == S.NW
    assert not res.view(np.uint32).any() and not fits[0]["a_re"].any() and not fits[0]["a_im"].any()


def test_two_decodes_are_subtracted_in_emission_order():
    """Two transmissions 21 Hz apart (their 83 Hz-wide tone sets interleave) and 0.08 s apart, equal strength.  Each is fitted from the ORIGINAL
    frame, so a decode's report does not depend on what is emitted beside it; the residual is frame - 2 y_0 - 2 y_1 in that order of float32
    operations, which the other order does not give bit for bit."""
    t2, t3 = SC.tones(SC.word(2)), SC.tones(SC.word(3))
    x = (SC.tx(2, 1500.9, 0.413, 700.0, 1.0) + SC.tx(3, 1521.2, 0.33, 700.0, 2.0)).astype(np.float32)
    i2, i3 = (t2, *SC.grid(1500.9, 0.413)), (t3, *SC.grid(1521.2, 0.33))
    recs, res, fits = S.subtract(x, [i2, i3])
    alone2, _, _ = S.subtract(x, [i2])
    alone3, _, _ = S.subtract(x, [i3])
    assert recs[0].tobytes() == alone2[0].tobytes() and recs[1].tobytes() == alone3[0].tobytes()
    y0, y1 = S.fitted_wave(fits[0]), S.fitted_wave(fits[1])
    want = x.copy()
    for f, y in ((fits[0], y0), (fits[1], y1)):
        want[f["start"]:f["start"] + S.NW] = want[f["start"]:f["start"] + S.NW] - np.float32(2.0) * y
    assert res.tobytes() == want.tobytes()
    recs_b, other, _ = S.subtract(x, [i3, i2])
    assert recs_b[0].tobytes() == recs[1].tobytes() and recs_b[1].tobytes() == recs[0].tobytes()
    assert other.tobytes() != res.tobytes() and np.allclose(other, res, atol=1e-2)
    # (not a joint fit: each sees the other, one tone spacing away, as interference of its own strength.  What is left is printed, not asserted)
    print("energy left: %.3f of the frame's" % (np.sum(res.astype(np.float64) ** 2) / np.sum(x.astype(np.float64) ** 2)))


# Removal depth, float32 restatement against the float64 implementation (tests/ft4_subtract_quality.py; profiles/ft4_subtract_quality.json holds
# the figures).  Measured over the twelve cases: db32 - db64 between -0.00001 and +0.0471 dB; the +0.047 is at the -54 dB floor of the on-grid
# noise-free case, where the 12-bit phase table and float32 sums begin to count; in noise the two agree to 0.001 dB.
# MARGIN: four times the largest difference measured, as DESIGN.md 4.15 set it for FT8.
MARGIN_DB = 4 * 0.0472


def test_removal_depth_float32_against_float64():
    rows = Q.measure()
    assert len(rows) == 12
    for r in rows:
        print("word %d f %.2f dt %.4f sigma %6.0f: float32 %.2f dB, float64 %.2f dB" % (r["word"], r["f_hz"], r["dt_s"], r["sigma"], r["db32"], r["db64"]))
    worst = max(r["db32"] - r["db64"] for r in rows)
    print("largest db32 - db64: %.4f dB (margin %.4f)" % (worst, MARGIN_DB))
    assert worst <= MARGIN_DB, worst
    assert all(r["db32"] < -30 for r in rows if r["sigma"] == 0)        # (the cases do remove something: noise-free, better than 30 dB)
