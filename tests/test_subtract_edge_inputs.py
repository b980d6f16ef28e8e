"""CPU: the inputs of tests/ft8_subtract_edge_cases.py and tests/ft4_subtract_edge_cases.py contain what they were made for, proved with the
restatements alone (tests/ft8_subtract_ref.py, tests/ft4_subtract_ref.py; never against the GPU) -- and they can SEE the errors they are aimed
at: a deliberately wrong restatement (an alignment remainder dropped, the FT4 pad-word select stuck at 0, a stale tail past n_valid, the records
applied in another order) differs from the true one in report bytes or residual words on the case meant for it.
The whole file takes about 12 s on one CPU core (measured: 10.4 to 12.5 s; the references of both modes, about 0.1 s per item, are most of it)."""
import numpy as np
import pytest

import ft4_subtract_edge_cases as E4
import ft4_subtract_ref as S4
import ft8_subtract_edge_cases as E8
import ft8_subtract_ref as S8

MODES = {"FT8": (S8, E8), "FT4": (S4, E4)}
F32 = np.float32
FIELDS = ("f_hz", "dt_s", "p_removed", "p_before", "p_after")
BOTH = pytest.mark.parametrize("mode", ["FT8", "FT4"])


def _w0(S, dt_s):
    """where sub_tile_pass starts tile 0's window"""
    return S.start_of(dt_s) - S.TAU_MAX


def _track(S, re, im, cnt):
    pre, pim, pc = (np.concatenate([np.zeros(S.HW, F32), v, np.zeros(S.HW, F32)]) for v in (re, im, cnt))
    nre, nim, den = np.zeros(S.NBLK, F32), np.zeros(S.NBLK, F32), np.zeros(S.NBLK, F32)
    for j in range(2 * S.HW + 1):
        nre, nim, den = nre + S.WIN[j] * pre[j:j + S.NBLK], nim + S.WIN[j] * pim[j:j + S.NBLK], den + S.WIN[j] * pc[j:j + S.NBLK]
    ok = den > 0
    with np.errstate(all="ignore"):
        return (np.where(ok, nre / np.where(ok, den, F32(1)), F32(0)).astype(F32), np.where(ok, nim / np.where(ok, den, F32(1)), F32(0)).astype(F32))


def _true_take(S, frame, i0):
    win = S._padded(frame, i0, -S.TAU_MAX, S.NW + S.TAU_MAX)
    return lambda it: win[it * S.TAU_STEP:it * S.TAU_STEP + S.NW]


def _fit(S, frame, tones, freq_hz, dt_s, take_of=_true_take):
    """S.fit written out with S's own pieces, the signal's samples at time offset `it` coming from take_of(S, frame, i0)(it): with _true_take it IS
    S.fit (test_the_local_fit_is_the_restatement); the wrong restatements below differ in take_of alone"""
    frame = np.asarray(frame, F32)
    i0 = S.start_of(dt_s)
    take = take_of(S, frame, i0)
    it0 = S.TAU_MAX // S.TAU_STEP
    inc = S.inc_of(freq_hz)
    ik = S.freq_search(*S.block_sums(take(it0), *S.wave(tones, inc)))
    inc = np.uint32((int(inc) + (ik - S.KF) * S.DINC) & 0xffffffff)
    c, s = S.wave(tones, inc)
    m = np.zeros(S.NTAU, F32)
    for it in range(S.NTAU):
        m[it] = S.symbol_metric(*S.block_sums(take(it), c, s))
    it = S.first_max(m)
    start = i0 - S.TAU_MAX + it * S.TAU_STEP
    ik2 = S.freq_search(*S.block_sums(take(it), c, s))
    inc = np.uint32((int(inc) + (ik2 - S.KF) * S.DINC) & 0xffffffff)
    t = start + np.arange(S.NW, dtype=np.int64)
    cnt = ((t >= 0) & (t < S.N)).reshape(S.NBLK, S.BLK).sum(axis=1).astype(F32)
    re, im = S.block_sums(take(it), *S.wave(tones, inc))
    a_re, a_im = _track(S, re, im, cnt)
    if hasattr(S, "slope_dinc"):                     # FT4: the track's own phase slope, then block sums and track once more
        inc = np.uint32((int(inc) + S.slope_dinc(a_re, a_im)) & 0xffffffff)
        re, im = S.block_sums(take(it), *S.wave(tones, inc))
        a_re, a_im = _track(S, re, im, cnt)
    with np.errstate(all="ignore"):
        okc = cnt > 0
        safe = np.where(okc, cnt, F32(1))
        removed = S.tree256(F32(2.0) * (a_re * a_re + a_im * a_im) * cnt)
        before = S.tree256(np.where(okc, F32(2.0) * (re * re + im * im) / safe, F32(0)).astype(F32))
        dr, di = re - cnt * a_re, im - cnt * a_im
        after = S.tree256(np.where(okc, F32(2.0) * (dr * dr + di * di) / safe, F32(0)).astype(F32))
    rec = np.zeros((), S.SUB_DTYPE)
    rec["f_hz"] = F32(np.float64(int(inc)) * (12000.0 / 4294967296.0))
    rec["dt_s"] = F32(start - 6000) / F32(12000.0)
    rec["p_removed"], rec["p_before"], rec["p_after"] = removed, before, after
    rec["n_inside"] = int(cnt.sum())
    rec["df_steps"], rec["dt_steps"] = (ik - S.KF) + (ik2 - S.KF), it - it0
    return rec, {"start": start, "inc": inc, "tones": np.asarray(tones, np.int64), "a_re": a_re, "a_im": a_im}


def _floored_take(S, frame, i0):
    """wrong restatement 1: the window's start floored to a multiple of 4 (the aligned load's address a0 taken for w0, the remainder r dropped)"""
    r = (i0 - S.TAU_MAX) % 4
    return _true_take(S, frame, i0 - r)


def _no_pad_select_take(S, frame, i0):
    """wrong restatement 2 (FT4): the kernel keeps the window in LDS with one pad word after every 18 and reads sample s of a block at padded word
    m0 + d0 + s + (r0 + s >= 18 ? 1 : 0), m0 = r + 2 it, d0 = m0 / 18, r0 = m0 mod 18.  With the select stuck at 0 the sample at r0 + s = 18 is the
    pad word (never written: taken as +0 here) and every later one of the block is the sample before the right one"""
    win = S._padded(frame, i0, -S.TAU_MAX, S.NW + S.TAU_MAX)
    r = (i0 - S.TAU_MAX) % 4

    def take(it):
        x = win[it * S.TAU_STEP:it * S.TAU_STEP + S.NW].reshape(S.NBLK, S.BLK).copy()
        r0 = (r + S.TAU_STEP * it) % S.BLK
        if r0:
            right = x.copy()
            x[:, S.BLK - r0 + 1:] = right[:, S.BLK - r0:-1]
            x[:, S.BLK - r0] = 0
        return x.reshape(-1)
    return take


def _items_of(E, name, frame=0):
    audio, items = E.kernel_cases()[name]
    idx = np.flatnonzero(items["frame"] == frame)
    return audio[frame], idx, [(E.tones(items["bits"][i]), items["freq_hz"][i], items["dt_s"][i]) for i in idx]


@BOTH
def test_the_local_fit_is_the_restatement(mode):
    S, E = MODES[mode]
    frame, idx, its = _items_of(E, "offgrid")
    sub, res, fits = E.kernel_fits("offgrid")
    for i, args in zip(idx, its):
        rec, f = _fit(S, frame, *args)
        assert rec.tobytes() == sub[i].tobytes()
        assert all(np.array_equal(f[k], fits[i][k]) for k in ("start", "inc", "a_re", "a_im"))


@BOTH
def test_offgrid(mode):
    S, E = MODES[mode]
    audio, items = E.kernel_cases()["offgrid"]
    sub, res, fits = E.kernel_fits("offgrid")
    assert audio.shape == (1, S.N) and len(items) == 4
    tone_hz = 12000.0 / S.NSPS
    assert min(abs(a - b) for i, a in enumerate(items["freq_hz"]) for b in items["freq_hz"][:i]) > 8 * tone_hz          # distinct frequencies
    w0 = [_w0(S, dt) for dt in items["dt_s"]]
    assert [w % 4 for w in w0] == [0, 1, 2, 3]
    # the starts the items were made for: the kernel's rounding of the float32 dt_s gives them back
    centre = [s + 6000 - S.CAND_STEP for k, f, s, d, a in E.OFFGRID] if mode == "FT8" else [s for k, f, s, d, a in E.OFFGRID]
    assert [S.start_of(dt) for dt in items["dt_s"]] == centre
    steps = [int(v) for v in sub["dt_steps"]]
    print(mode, "offgrid: w0 mod 4", [w % 4 for w in w0], "dt_steps", steps, "df_steps", [int(v) for v in sub["df_steps"]])
    assert sum(1 for v in steps if v != 0) >= 2
    # the winners are where the transmissions were put and inside the search's reach.  (To one block, 1/32 of a symbol: the metric is a sum of
    # |symbol sum|^2, which falls off by about the fraction of a symbol the start is wrong by, so its top is flat and noise moves it by a few
    # samples.)
    for (k, f, s, d, a), v in zip(E.OFFGRID, steps):
        assert abs(v * S.TAU_STEP - d) <= S.BLK and abs(v) < S.TAU_MAX // S.TAU_STEP
    assert (sub["n_inside"] == S.NW).all() and (sub["p_after"] < 0.2 * sub["p_before"]).all()
    if mode == "FT4":
        # the remainder the pad-word select sees at the winner: r0 = (r + 2 it) mod 18, odd on two items
        r0 = [(w % 4 + S.TAU_STEP * (v + S.TAU_MAX // S.TAU_STEP)) % S.BLK for w, v in zip(w0, steps)]
        assert sum(1 for v in r0 if v % 2) >= 2, r0
    assert np.isfinite([[float(sub[i][f]) for f in FIELDS] for i in range(4)]).all()


@BOTH
def test_offgrid_sees_a_dropped_remainder(mode):
    S, E = MODES[mode]
    frame, idx, its = _items_of(E, "offgrid")
    sub, res, fits = E.kernel_fits("offgrid")
    wrong = [_fit(S, frame, *args, take_of=_floored_take) for args in its]
    differs = [rec.tobytes() != sub[i].tobytes() for i, (rec, f) in zip(idx, wrong)]
    assert differs == [False, True, True, True]                          # (r = 0: the same window)
    assert (S.apply(frame, [f for rec, f in wrong]).view(np.uint32) != res[0].view(np.uint32)).any()


def test_offgrid_sees_a_stuck_pad_select():
    """(FT4 alone: the FT8 kernel indexes its padded window without a select)"""
    S, E = S4, E4
    frame, idx, its = _items_of(E, "offgrid")
    sub, res, fits = E.kernel_fits("offgrid")
    odd = [i for i in idx if _w0(S, its[i][2]) % 2]
    assert len(odd) == 2
    for i in odd:
        rec, f = _fit(S, frame, *its[i], take_of=_no_pad_select_take)
        assert rec.tobytes() != sub[i].tobytes()
        assert (S.apply(frame, [f]).view(np.uint32) != S.apply(frame, [fits[i]]).view(np.uint32)).any()


@BOTH
def test_limits(mode):
    S, E = MODES[mode]
    audio, items = E.kernel_cases()["limits"]
    sub, res, fits = E.kernel_fits("limits")
    assert audio.shape == (1, S.N) and len(items) == 7
    assert list(items["dt_s"][:2]) == [30.0, -30.0] and list(items["freq_hz"][4:6]) == [0.0, 6000.0]
    assert np.isfinite([[float(sub[i][f]) for f in FIELDS] for i in range(7)]).all() and np.isfinite(res).all()
    # wholly outside: nothing inside, the three energies +0 (bits and all), the first maximum of two all-zero metrics
    for i in (0, 1):
        assert sub["n_inside"][i] == 0
        assert all(sub[f][i].tobytes() == F32(0).tobytes() for f in ("p_removed", "p_before", "p_after"))
        assert (sub["df_steps"][i], sub["dt_steps"][i]) == (-2 * S.KF, -(S.TAU_MAX // S.TAU_STEP))
        recs, alone, _ = S.subtract(audio[0], [(E.tones(items["bits"][i]), items["freq_hz"][i], items["dt_s"][i])])
        assert alone.tobytes() == audio[0].tobytes() and recs[0].tobytes() == sub[i].tobytes()
    # the slivers: less than a block inside, one at the frame's end (the signal's first samples), one at its start (the signal's last)
    assert (0 < sub["n_inside"][2] < S.BLK) and (0 < sub["n_inside"][3] < S.BLK)
    assert fits[2]["start"] > S.N - S.BLK and fits[3]["start"] + S.NW < S.BLK
    # freq_hz = 0: the search steps the increment below 0 and f_hz reports the wrapped one, just under 12000; 6000 stays near 6000
    assert sub["df_steps"][4] < 0 and 11990.0 < sub["f_hz"][4] < 12000.0
    assert abs(sub["f_hz"][5] - 6000.0) < 5.0
    print(mode, "limits:", [(float(sub["f_hz"][i]), int(sub["n_inside"][i]), int(sub["df_steps"][i]), int(sub["dt_steps"][i])) for i in range(7)])
    # the real transmission, last: found, and taken out as if it stood alone -- or not: the byte comparison on the device settles that; here
    # only that the six before it did not keep the fit from it (a fit reads the ORIGINAL frame)
    assert sub["n_inside"][6] == S.NW and sub["p_after"][6] < 0.2 * sub["p_before"][6]
    recs, alone, _ = S.subtract(audio[0], [(E.tones(items["bits"][6]), items["freq_hz"][6], items["dt_s"][6])])
    assert recs[0].tobytes() == sub[6].tobytes()


@BOTH
def test_crowded_and_reversed(mode):
    S, E = MODES[mode]
    audio, items = E.kernel_cases()["crowded"]
    sub, res, fits = E.kernel_fits("crowded")
    assert audio.shape == (8, S.N) and len(items) == 27
    assert {f: int((items["frame"] == f).sum()) for f in (0, 3, 7)} == {0: 1, 3: 24, 7: 2} == E.CROWD_COUNTS
    assert E.offsets_table("crowded") == [0, 1, 1, 1, 25, 25, 25, 25]     # equal offsets in the middle and up to the end
    for f in (1, 2, 4, 5, 6):
        assert res[f].tobytes() == audio[f].tobytes()
    # frame 3: twelve transmissions, each named twice, the second time 1 Hz and 3 samples away
    on3 = items[items["frame"] == 3]
    assert len({b.tobytes() for b in on3["bits"]}) == 12
    assert all(on3["bits"][i].tobytes() == on3["bits"][i + 12].tobytes() and on3["freq_hz"][i + 12] == on3["freq_hz"][i] + 1.0
               and S.start_of(on3["dt_s"][i + 12]) == S.start_of(on3["dt_s"][i]) + 3 for i in range(12))
    # four of them pairwise within one tone spacing and overlapping in time
    four = E.CROWD[:4]
    assert max(f for k, f, s, a in four) - min(f for k, f, s, a in four) < E.TONE_HZ
    assert max(s for k, f, s, a in four) - min(s for k, f, s, a in four) < S.NW // 4
    assert np.isfinite([[float(sub[i][f]) for f in FIELDS] for i in range(27)]).all()
    # the fits find them: the first naming of every transmission without a neighbour within a tone lands on it: within half a hertz, and the time search's
    # winner is not at an end of its grid
    for i, (k, f, s0, a) in zip(range(5, 13), E.CROWD[4:]):
        assert abs(float(sub["f_hz"][i]) - f) < 0.5 and abs(int(sub["dt_steps"][i])) < S.TAU_MAX // S.TAU_STEP, (i, sub[i])
    # trailing: one item on the first of three frames
    assert E.offsets_table("trailing") == [0, 1, 1] and len(E.kernel_cases()["trailing"][1]) == 1

    # reversed: frame 3 alone, its items in reverse order; the same fits (a fit reads the original frame), another residual
    raudio, ritems = E.kernel_cases()["reversed"]
    rsub, rres, rfits = E.kernel_fits("reversed")
    assert raudio.shape == (1, S.N) and raudio[0].tobytes() == audio[3].tobytes() and len(ritems) == 24
    assert all(ritems["bits"][i].tobytes() == on3["bits"][23 - i].tobytes() and ritems["freq_hz"][i] == on3["freq_hz"][23 - i]
               and ritems["dt_s"][i] == on3["dt_s"][23 - i] for i in range(24))
    # (the case module takes the reversed case's fits from the forward one's; the restatement on the reversed items themselves agrees)
    for i in (0, 23):
        rec, f = S.fit(raudio[0], E.tones(ritems["bits"][i]), ritems["freq_hz"][i], ritems["dt_s"][i])
        assert rec.tobytes() == rsub[i].tobytes() and np.array_equal(f["a_re"], rfits[i]["a_re"]) and f["start"] == rfits[i]["start"]
    n_diff = int((rres[0].view(np.uint32) != res[3].view(np.uint32)).sum())
    print(mode, "reversed: residual words that differ from the forward order's:", n_diff)
    assert n_diff > 0
    # wrong restatement 4: the records applied in the order of their frequencies instead of the order of emission
    for name, frame, own, ref in (("crowded", audio[3], fits[1:25], res[3]), ("reversed", raudio[0], rfits, rres[0])):
        by_freq = sorted(own, key=lambda f: int(f["inc"]))
        assert (S.apply(frame, by_freq).view(np.uint32) != ref.view(np.uint32)).any(), name


@BOTH
def test_a_stale_tail_is_seen(mode):
    """The chain's short slot (tests/test_gpu_subtract_ft8.py, tests/test_gpu_subtract_ft4.py): the reference there is the restatement on the frame
    with +0 from n_valid on.  On a synthetic frame whose tail holds another transmission's samples -- what an earlier slot leaves in the device
    buffer -- a subtractor that keeps the tail as found (wrong restatement 3), in the fit or in the apply alone, gives other reports or another
    residual; n_valid lies inside the signal and is no multiple of 4."""
    S, E = MODES[mode]
    first = 13000 if mode == "FT8" else 7000                            # the signal's first sample
    rel = first - 6000 if mode == "FT8" else first                      # (as the case modules' sent() and at() count it)
    n_valid = first + S.NW - 3 * S.NSPS - 1
    assert n_valid % 4 != 0 and first < n_valid < first + S.NW
    stale = E.sent(70, 1500.0, rel, 600.0) + E.sent(71, 1480.0, rel - 900, 900.0) + E.noise(71, 100.0)
    stale = np.asarray(stale, F32)
    true = stale.copy()
    true[n_valid:] = 0
    assert stale[n_valid:].any()
    it = E.at(0, 70, E.grid_hz(1500.0), rel + (S.CAND_STEP if mode == "FT8" else 0))
    args = [(E.tones(it["bits"]), it["freq_hz"], it["dt_s"])]
    recs, res, fits = S.subtract(true, args)
    assert not res[first + S.NW + S.TAU_MAX:].any() and res[n_valid:first + S.NW - S.TAU_MAX].any()          # past n_valid the residual is 0 - 2 y
    wrecs, wres, wfits = S.subtract(stale, args)                                      # no mask at all
    assert wrecs[0].tobytes() != recs[0].tobytes() and (wres.view(np.uint32) != res.view(np.uint32)).any()
    assert (S.apply(stale, fits).view(np.uint32) != res.view(np.uint32)).any()        # the fit masked, the apply not
    assert (S.apply(true, wfits).view(np.uint32) != res.view(np.uint32)).any()        # the apply masked, the fit not
