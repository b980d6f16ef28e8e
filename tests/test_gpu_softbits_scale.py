"""GPU: the machinery AROUND the three soft-bit / refinement stages (ft8_softbits_kernel, ft4_refine_kernel, ft4_softbits_kernel) -- which record
array a workgroup writes, when the arrays are reallocated, what a fetch hands out afterwards -- driven through the C ABI of the product library
into the states the arithmetic tests (tests/test_gpu_ft8_softbits.py, tests/test_gpu_ft4_softbits.py) never reach: many FT4 channels in one
boundary, both features in one context, reconfiguration with a feature on, channels that come and go, degenerate and wide launch shapes, and
cwslg_fetch_slot next to the soft-bit fetches.

Standard of comparison everywhere: BIT-EXACT, none skipped.  The candidate lists equal oracle.ft8_sync / oracle.ft4_candidates of the GPU's own
int16 frame, the FT4 sync records equal oracle.ft4_sync_all(frame, list), llr and sigma equal the numpy restatements (tests/ft8_softbits_ref.py,
tests/ft4_softbits_ref.py) as uint32, nsync and nqual as integers.  The signal recipes come from tests/softbits_cases.py;
tests/test_softbits_scale_inputs.py shows on the CPU, with the oracle's own chain, that each recipe meets the conditions asserted here again on
the library's output (bursts found with nsync 21 / 16 and no wrong sign, edge records, list lengths), so no test can pass by producing too
little to compare.

Wall times: NOT YET RECORDED.  At the time of this commit the module had been collected and its recipes vetted on the CPU, but it had not run on
an MI355X; the first GPU run must record each test's wall time here (the yardstick is a few seconds each, well under a minute in all; the host
side of it -- oracle and restatements on the compared channels -- takes about 40 s for all nine cases together, measured through the CPU module).
"""
import numpy as np
import pytest

import ft4_softbits_ref as R4
import ft8_softbits_ref as R8
import softbits_cases as S

pytestmark = pytest.mark.gpu
FS, BLK, N4, N8 = S.FS, S.BLK, S.N4, S.N8
U32 = np.uint32
ERR_ARG = -6


@pytest.fixture
def xctx():
    """A fresh context in the default (exact) arithmetic mode."""
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


def _push(ctx, rx, iq):
    iq = np.ascontiguousarray(iq, dtype=np.complex64)
    for k in range(0, len(iq), 64 * BLK):
        ctx.push_iq(rx, iq[k:k + 64 * BLK])


def _start(ctx, e):
    ctx.slot_boundary("FT8", e); ctx.slot_boundary("FT4", e)


def _pair(ctx, rx, iq, e, after_mid=None):
    """One pair slot that began at epoch e: the FT4 group's boundary in the middle (e + 8), then both groups' at e + 15, FT8 first.
    -> (start epoch of the FT8 frame, start epoch of the second FT4 frame)"""
    _push(ctx, rx, iq[:N4])
    ctx.slot_boundary("FT4", e + 8)
    if after_mid:
        after_mid()
    _push(ctx, rx, iq[N4:])
    ctx.slot_boundary("FT8", e + 15); ctx.slot_boundary("FT4", e + 15)
    return e, e + 8


def _key(cands):
    return [(c[0], c[1], int(np.float32(c[2]).view(U32)), int(np.float32(c[3]).view(U32)), float(c[4])) for c in cands]


def _check8(ctx, oracle, ch, t_start=None, f_hi=3000, max_cand=200, syncmin=1.5, order="sync", plane_too=False):
    """Frame, list and FT8 soft records of one epoch: the list is the oracle's, the row pitch the feature's, every record the restatement's."""
    fr = ctx.fetch_frame(ch)
    cands, t_c = ctx.fetch_candidates(ch, 600, with_epoch=True)
    got = ctx.fetch_ft8_softbits(ch, 600, with_epoch=True)
    assert got is not None, "no FT8 soft-bit records of the current epoch"
    llr, sigma, nsync, t_s = got
    assert t_s == t_c == fr["t_start"] and (t_start is None or t_s == t_start), (t_s, t_c, fr["t_start"], t_start)
    assert _key(cands) == _key(oracle.ft8_sync(fr["i16"], 200, f_hi, syncmin, max_cand, order=order))
    g = ctx.sync_debug(ch, "spectra")
    pitch = R8.soft_pitch(f_hi)
    assert g.shape == (372, pitch), g.shape
    ref = S.ft8_reference(oracle, fr["i16"], cands, pitch)
    if plane_too:
        assert np.array_equal(g.view(U32), ref["plane"].view(U32))
    assert llr.shape == ref["llr"].shape == (len(cands), 174) and len(cands) <= max_cand, (llr.shape, len(cands))
    bad = np.nonzero((llr.view(U32) != ref["llr"].view(U32)).any(axis=1) | (sigma.view(U32) != ref["sigma"].view(U32)) | (nsync != ref["nsync"]))[0]
    assert bad.size == 0, (bad[:5], [cands[q][:2] for q in bad[:5]])
    return dict(fr=fr, cands=cands, llr=llr, sigma=sigma, nsync=nsync)


def _check4(ctx, oracle, ch, t_start=None, f_lo=200, f_hi=3000, max_cand=100, order="sync"):
    """Frame, list, FT4 sync records and FT4 soft records of one epoch against the oracle and the restatement, every record, every field."""
    fr = ctx.fetch_frame(ch)
    cands, t_c = ctx.fetch_candidates(ch, 600, with_epoch=True)
    recs = ctx.fetch_ft4_sync(ch, 1800)
    got = ctx.fetch_ft4_softbits(ch, 1800, with_epoch=True)
    assert got is not None, "no FT4 soft-bit records of the current epoch"
    llr, sigma, nsync, nqual, t_s = got
    assert t_s == t_c == fr["t_start"] and (t_start is None or t_s == t_start), (t_s, t_c, fr["t_start"], t_start)
    assert _key(cands) == _key(oracle.ft4_candidates(fr["i16"], float(f_lo), float(f_hi), 1.2, max_cand, order=order))
    ref = S.ft4_reference(oracle, fr["i16"], cands)
    assert recs == ref["recs"]
    assert all(0 <= h["cand"] < min(max_cand, len(cands)) for h in recs)
    assert llr.shape == ref["llr"].shape == (len(recs), 3, 174) and sigma.shape == ref["sigma"].shape, (llr.shape, len(recs))
    bad = np.nonzero((llr.view(U32) != ref["llr"].view(U32)).any(axis=(1, 2)) | (sigma.view(U32) != ref["sigma"].view(U32)).any(axis=1)
                     | (nsync != ref["nsync"]) | (nqual != ref["nqual"]))[0]
    assert bad.size == 0, (bad[:5], [recs[q] for q in bad[:3]])
    return dict(fr=fr, cands=cands, recs=recs, llr=llr, sigma=sigma, nsync=nsync, nqual=nqual, cx=ref["cx"])


def _closed(ctx, ch, fetch):
    from cwsl_digi_amd.api import CwslGpuError
    with pytest.raises(CwslGpuError) as e:
        fetch(ch)
    assert e.value.status == ERR_ARG


def test_ft4_many_channels_one_boundary(ctx, oracle):
    """Gap 1, FT4 at more than two channels per boundary: 37 FT4 channels (an odd count) on one receiver finalise in ONE boundary, so sync_launch
    builds works4c and soft4 with 37 entries each and uploads the pointer table behind the 37 descriptors (wb4_bytes); ft4_refine_kernel runs on the
    grid (max_cand = 100, 37) and ft4_softbits_kernel on (300, 37), each workgroup taking works + blockIdx.y and soft[blockIdx.y].  Six probe
    channels (first, last, the adjacent 17 / 18, 9 and 27) carry two or three bursts at their own frequencies and start times; the records and soft
    records of the probes and of two noise-only channels are the oracle's and the restatement's, every probe burst is found, and no probe channel
    holds a strong record at another probe's frequency -- a table in the wrong order or a stride error would put one there."""
    iq, tones = S.many_channels_iq(oracle)
    ctx.enable_sync(True, 1.5, 100, 200, 3000)
    ctx.enable_ft4_coherent(True)
    ctx.enable_ft4_softbits(True)
    rx = ctx.receiver_open(FS, BLK, 0)
    chans = [ctx.channel_open(rx, f, "FT4") for f in S.MANY_DIALS]
    assert len(chans) == 37
    ctx.slot_boundary("FT4", 10)
    before = ctx.stats()["sync_launches"]
    _push(ctx, rx, iq)
    ctx.slot_boundary("FT4", 17)
    assert ctx.stats()["sync_launches"] - before == 1                     # all 37 in one launch
    for p, bursts in S.MANY_PROBES.items():
        r = _check4(ctx, oracle, chans[p], 10)
        S.assert_ft4_found(r["recs"], r["llr"], r["nsync"], bursts, tones[("FT4", S.MANY_DIALS[p])])
        S.assert_no_foreign_record(r["recs"], p)
    for k in S.MANY_NOISE_ONLY:
        r = _check4(ctx, oracle, chans[k], 10)
        S.assert_no_foreign_record(r["recs"], None)


def test_both_features_ft8_and_ft4_together(xctx, oracle):
    """Gap 2, both features on in one context: 5 FT8 and 3 FT4 channels on one receiver, cwslg_enable_ft8_softbits and cwslg_enable_ft4_softbits
    both on, so that sync_ensure_channel decides the FT8 channels' allocation from cfg.ft8_soft (row pitch cfg.nbins, d_soft behind the list) while
    the FT4 channels keep FT4_ROW and get their record arrays from ensure_record_array.

    One boundary CANNOT carry both groups: cwslg_slot_boundary and cwslg_slot_boundary_begin collect `c->chans[k].group == group` only, FT8 and FT4
    are groups 0 and 1 (cwslg_slot_boundary_channel takes one channel), and boundary_locked calls sync_launch with the ids it was given.  n8 > 0 with
    n4 > 0 in one sync_launch -- the FT8 pointer table at `wb->d + n8 + n4` with n4 != 0 -- is therefore unreachable through the C ABI; the two groups'
    boundaries are driven back to back at one epoch instead (FT8 first, then FT4), which is what a host does at every second FT4 slot.

    Slot 1 both on: FT8 soft records on every FT8 channel, pitch 992 and the `spectra` plane against oracle.ft8_spectra; FT4 sync and soft records on
    every FT4 channel, whose `spectra` plane keeps its (122, 1168) shape.  Slot 2 with FT8 soft bits off, FT4 on: the FT8 fetch is None ("after a
    boundary that ran with the feature off there is nothing to fetch", include/cwsl_gpu.h), the FT8 pitch is back to ib + 13 rounded up (sync_host.inc,
    cwslg_enable_ft8_softbits: `cfg.nbins = (cfg.ib + (cfg.ft8_soft ? 15 : 13) + 31) / 32 * 32`; f_hi = 2959 makes that 960 against 992), the FT4
    records of the new slot are exact.  Slot 3 the reverse."""
    ctx = xctx
    f_hi = 2959
    ctx.enable_sync(True, 1.5, 100, 200, f_hi)
    ctx.enable_ft8_softbits(True)
    ctx.enable_ft4_softbits(True)
    rx = ctx.receiver_open(FS, BLK, 0)
    c8 = [ctx.channel_open(rx, f, "FT8") for f in S.BOTH_FT8_DIALS]
    c4 = [ctx.channel_open(rx, f, "FT4") for f in S.BOTH_FT4_DIALS]
    e = 1
    _start(ctx, e)

    def run(k):
        nonlocal e
        seed, ft8, ft4 = S.both_slot(k)
        iq, tones = S.pair_iq(oracle, seed, ft8, ft4)
        t8, t4 = _pair(ctx, rx, iq, e)
        e += 15
        return t8, t4, ft8, ft4, tones

    def all8(t8, ft8, tones):
        for ch, (dial, bursts) in zip(c8, ft8):
            r = _check8(ctx, oracle, ch, t8, f_hi=f_hi, max_cand=100, plane_too=True)
            S.assert_ft8_found(r["cands"], r["llr"], r["nsync"], bursts, tones[("FT8", dial)])

    def all4(t4, ft4, tones):
        for ch, (dial, bursts) in zip(c4, ft4):
            r = _check4(ctx, oracle, ch, t4, f_hi=f_hi)
            S.assert_ft4_found(r["recs"], r["llr"], r["nsync"], bursts, tones[("FT4", dial)])
            assert ctx.sync_debug(ch, "spectra").shape == (122, 1168)

    t8, t4, ft8, ft4, tones = run(0)
    assert R8.soft_pitch(f_hi) == 992
    all8(t8, ft8, tones); all4(t4, ft4, tones)
    ctx.enable_ft8_softbits(False)                                        # FT8 off, FT4 stays on
    t8, t4, ft8, ft4, tones = run(1)
    for ch in c8:
        assert ctx.fetch_ft8_softbits(ch) is None
        assert ctx.sync_debug(ch, "spectra").shape == (372, 960)
        fr = ctx.fetch_frame(ch)
        cands, t_c = ctx.fetch_candidates(ch, 600, with_epoch=True)
        assert t_c == fr["t_start"] == t8 and _key(cands) == _key(oracle.ft8_sync(fr["i16"], 200, f_hi, 1.5, 100)) and len(cands) >= 2
    all4(t4, ft4, tones)
    ctx.enable_ft8_softbits(True); ctx.enable_ft4_softbits(False)         # the reverse
    t8, t4, ft8, ft4, tones = run(2)
    all8(t8, ft8, tones)
    for ch, (dial, bursts) in zip(c4, ft4):
        assert ctx.fetch_ft4_softbits(ch) is None
        fr = ctx.fetch_frame(ch)
        cands, t_c = ctx.fetch_candidates(ch, 600, with_epoch=True)
        assert t_c == fr["t_start"] == t4 and ctx.fetch_ft4_sync(ch) == oracle.ft4_sync_all(fr["i16"], cands) and len(cands) >= 2


def test_reconfigure_between_slots_with_soft_bits_on(xctx, oracle):
    """Gap 3, reconfiguration while a feature is on: one FT8 and one FT4 channel, both features on, six pair slots with different signals;
    before each slot cwslg_enable_sync is called again -- max_cand 100 -> 7 -> 200, then f_hi 3000 -> 2959 -> 3100 (FT8 pitch 992 -> 992 -> 1024,
    checked against ft8_softbits_ref.soft_pitch), candidate order "freq" for the fifth slot and "sync" again for the sixth -- so that
    sync_ensure_channel frees and reallocates everything (`b.max_cand == cfg.max_cand`, `b.nbins == want_bins` fail), d_soft included, and
    ensure_record_array's caller sizes the FT4 array again from b.max_cand.

    Contract of a re-enable, from sync_host.inc, cwslg_enable_sync: `cfg.kept = c->sync_cfg.kept;` (SyncConfig::Kept holds ft8_soft and ft4_soft)
    and `if (cfg.kept.ft8_soft) cfg.nbins = (cfg.ib + 15 + 31) / 32 * 32;` -- the features stay on and the pitch is recomputed; asserted here by the
    records being there after the next boundary without another enable call.
    Between the re-enable and the next boundary the previous slot's records are HANDED OUT UNCHANGED: nothing is reallocated before the boundary
    (sync_launch -> sync_ensure_channel), the epochs still agree, and the fetches size themselves by the channel's own buffers
    (fetch_begin: `ch.syncbuf.max_cand` is the source's `cap`; fetch_flat: `lim = std::min(std::max(max, 0), s.cap);`, fetch_walk: `std::min(cnt, s.cap)`),
    not by the new configuration -- so the count cannot shrink to the new max_cand nor the contents change.

    After every slot: list, FT4 records and both kinds of soft records exact, record counts inside the current max_cand, each fetch under the
    frame's epoch, the probe bursts found."""
    ctx = xctx
    rx = ctx.receiver_open(FS, BLK, 0)
    c8 = ctx.channel_open(rx, S.RECONF_FT8_DIAL, "FT8")
    c4 = ctx.channel_open(rx, S.RECONF_FT4_DIAL, "FT4")
    e = 1
    prev = None
    for k, (max_cand, f_hi, order) in enumerate(S.RECONF_CONFIG):
        ctx.enable_sync(True, 1.5, max_cand, 200, f_hi)
        ctx.set_candidate_order(order)
        if k == 0:
            ctx.enable_ft8_softbits(True); ctx.enable_ft4_softbits(True)   # once: every later enable_sync must keep them
            _start(ctx, e)
        else:
            g8, g4 = ctx.fetch_ft8_softbits(c8, 600, with_epoch=True), ctx.fetch_ft4_softbits(c4, 1800, with_epoch=True)
            assert g8 is not None and g4 is not None
            assert g8[3] == prev[0]["fr"]["t_start"] and g4[4] == prev[1]["fr"]["t_start"]
            for got, want in zip(g8[:3], (prev[0]["llr"], prev[0]["sigma"], prev[0]["nsync"])):
                assert got.shape == want.shape and np.array_equal(got.view(U32), want.view(U32))
            for got, want in zip(g4[:4], (prev[1]["llr"], prev[1]["sigma"], prev[1]["nsync"], prev[1]["nqual"])):
                assert got.shape == want.shape and np.array_equal(got.view(U32), want.view(U32))
            assert _key(ctx.fetch_candidates(c8, 600)) == _key(prev[0]["cands"]) and ctx.fetch_ft4_sync(c4) == prev[1]["recs"]
        seed, ft8, ft4 = S.reconf_slot(k)
        iq, tones = S.pair_iq(oracle, seed, ft8, ft4)
        t8, t4 = _pair(ctx, rx, iq, e)
        e += 15
        r8 = _check8(ctx, oracle, c8, t8, f_hi=f_hi, max_cand=max_cand, order=order)
        r4 = _check4(ctx, oracle, c4, t4, f_hi=f_hi, max_cand=max_cand, order=order)
        assert ctx.sync_debug(c8, "spectra").shape[1] == R8.soft_pitch(f_hi) == (1024 if f_hi == 3100 else 992)
        assert len(r8["cands"]) <= max_cand and len(r4["cands"]) <= max_cand and len(r4["recs"]) <= 3 * max_cand
        if max_cand == 7:
            assert len(r8["cands"]) == len(r8["llr"]) == 7 and len(r4["cands"]) == 7 and max(h["cand"] for h in r4["recs"]) < 7
            assert len(oracle.ft8_sync(r8["fr"]["i16"], 200, f_hi, 1.5, 200)) > 7
            assert len(oracle.ft4_candidates(r4["fr"]["i16"], 200.0, float(f_hi), 1.2, 100)) > 7
        if order == "freq":
            assert [c[0] for c in r8["cands"]] == sorted(c[0] for c in r8["cands"])
        S.assert_ft8_found(r8["cands"], r8["llr"], r8["nsync"], ft8[0][1][:2], tones[("FT8", ft8[0][0])][:2])
        S.assert_ft4_found(r4["recs"], r4["llr"], r4["nsync"], ft4[0][1][:2], tones[("FT4", ft4[0][0])][:2])
        prev = (r8, r4)


def test_channels_open_and_close_between_slots(xctx, oracle):
    """Gap 4, channels that come and go: works8, works4c, soft8 and soft4 are rebuilt per boundary in the order of `emitted` (sync_launch), so
    after a close and an open every surviving channel must still receive its own records.  Both features on.  Slot 1: FT8 channels A, B, C and FT4
    channels P, Q, R, each with its own signals.  A and P are closed, D (FT8) and S (FT4) opened at new frequencies.  Slot 2, new signals: B, C, D,
    Q, R, S hold exactly their own records (parity and found bursts).  Then every FT4 channel is closed: slot 3's FT8 records are still exact and
    the FT4 group's boundaries have nothing to do.

    A closed id is an error, not old data: every fetch begins with `if (ch_id < 0 || ch_id >= (int)c->chans.size() || !c->chans[ch_id].open)
    return fail(c, CWSLG_ERR_ARG, "bad channel id");` (sync_host.inc) and cwslg_channel_close ends with `ch = Channel();` behind
    sync_free_channel(ch.syncbuf).
    A channel opened mid-stream has nothing to fetch (None: `if (!ch.have_frame ...) return CWSLG_ERR_NO_FRAME;`) until its first complete slot: a
    frame is emitted only if the buffer it filled was given a start epoch by an earlier boundary (boundary_locked: `f.emit = (ch.t0[cur] != 0)`).
    S gets that from the FT4 group's boundary in the middle of slot 2, whose frame -- begun before S was opened, no epoch -- is discarded; D gets it
    from cwslg_slot_boundary_channel right after it is opened, the call a host makes for a channel that joins at a slot's start."""
    ctx = xctx
    ctx.enable_sync(True, 1.5, 100, 200, 3000)
    ctx.enable_ft8_softbits(True)
    ctx.enable_ft4_softbits(True)
    rx = ctx.receiver_open(FS, BLK, 0)
    ids = {c: ctx.channel_open(rx, S.CHURN_DIALS[c], "FT8" if c in "ABCD" else "FT4") for c in "ABCPQR"}
    e = 1
    _start(ctx, e)

    def check(k, t8, t4, names8, names4, ft8, ft4, tones):
        for c, (dial, bursts) in zip(names8, ft8):
            r = _check8(ctx, oracle, ids[c], t8, max_cand=100)
            S.assert_ft8_found(r["cands"], r["llr"], r["nsync"], bursts, tones[("FT8", dial)])
        for c, (dial, bursts) in zip(names4, ft4):
            r = _check4(ctx, oracle, ids[c], t4)
            S.assert_ft4_found(r["recs"], r["llr"], r["nsync"], bursts, tones[("FT4", dial)])

    seed, names8, names4, ft8, ft4 = S.churn_slot(0)
    iq, tones = S.pair_iq(oracle, seed, ft8, ft4)
    t8, t4 = _pair(ctx, rx, iq, e); e += 15
    check(0, t8, t4, names8, names4, ft8, ft4, tones)

    a, p = ids.pop("A"), ids.pop("P")
    ctx.channel_close(a); ctx.channel_close(p)
    for fetch in (ctx.fetch_ft8_softbits, ctx.fetch_ft4_softbits, ctx.fetch_candidates, ctx.fetch_ft4_sync):
        _closed(ctx, a, fetch); _closed(ctx, p, fetch)
    ids["D"] = ctx.channel_open(rx, S.CHURN_DIALS["D"], "FT8")
    ids["S"] = ctx.channel_open(rx, S.CHURN_DIALS["S"], "FT4")
    ctx.slot_boundary_channel(ids["D"], e)
    assert ctx.fetch_ft8_softbits(ids["D"]) is None and ctx.fetch_ft4_softbits(ids["S"]) is None

    def mid():
        assert ctx.fetch_ft4_softbits(ids["S"]) is None and ctx.fetch_frame(ids["S"]) is None      # its first boundary: the frame had no epoch
        assert ctx.fetch_ft8_softbits(ids["D"]) is None and ctx.fetch_frame(ids["D"]) is None
    seed, names8, names4, ft8, ft4 = S.churn_slot(1)
    iq, tones = S.pair_iq(oracle, seed, ft8, ft4)
    t8, t4 = _pair(ctx, rx, iq, e, after_mid=mid); e += 15
    check(1, t8, t4, names8, names4, ft8, ft4, tones)

    closed4 = [ids.pop(c) for c in "QRS"]
    for ch in closed4:
        ctx.channel_close(ch)
    before = ctx.stats()["sync_launches"]
    seed, names8, names4, ft8, ft4 = S.churn_slot(2)
    iq, tones = S.pair_iq(oracle, seed, ft8, ft4)
    t8, t4 = _pair(ctx, rx, iq, e); e += 15
    assert ctx.stats()["sync_launches"] - before == 1                     # the FT8 group's; the FT4 group's two boundaries found no channel
    check(2, t8, t4, names8, names4, ft8, ft4, tones)
    for ch in closed4:
        _closed(ctx, ch, ctx.fetch_ft4_softbits)


def test_ft8_soft_small_and_large_lists(xctx, oracle):
    """Gap 5 (launch shapes, lists): ft8_softbits_kernel takes four candidates per workgroup, grid ((max_cand + 3) / 4, n8) -- max_cand 1, 2, 3 are
    less than one workgroup, 600 is 150 of them; the candidate count is read on the device, so a slot with many candidates followed by one with few
    in the same buffers must hand out the second list's records and count only.  One four-signal FT8 channel at max_cand 1, 2, 3 (record count =
    list length = max_cand, every record exact); 16 signals at max_cand 600 and syncmin 1.2 (more than 200 entries, the list not cut); then, with
    unchanged configuration, 12 signals followed by 1, and on an FT4 channel 6 bursts followed by 1: the second fetch returns exactly the second
    list's count (cwslg_fetch_ft8_softbits: `cnt = std::max(0, std::min(cnt, lim));`), every record is the second slot's, and a fetch that asks
    for more than the count gets the count."""
    ctx = xctx
    d8, d4 = S.LISTS_FT8_DIAL, S.LISTS_FT4_DIAL
    rx = ctx.receiver_open(FS, BLK, 0)
    c8 = ctx.channel_open(rx, d8, "FT8")
    e = 1
    iq4, _ = S.build_iq(oracle, 340, N8, ft8=[(d8, S.LISTS_FOUR)])
    for k, max_cand in enumerate((1, 2, 3)):
        ctx.enable_sync(True, 1.5, max_cand, 200, 3000)
        if k == 0:
            ctx.enable_ft8_softbits(True); ctx.enable_ft4_softbits(True)
            _start(ctx, e)
        t8, _ = _pair(ctx, rx, iq4, e); e += 15
        r = _check8(ctx, oracle, c8, t8, max_cand=max_cand)
        assert len(r["cands"]) == len(r["llr"]) == max_cand and len(oracle.ft8_sync(r["fr"]["i16"], 200, 3000, 1.5, 600)) > 3
    ctx.enable_sync(True, 1.2, 600, 200, 3000)
    iq, _ = S.build_iq(oracle, 341, N8, ft8=[(d8, S.LISTS_DENSE)])
    t8, _ = _pair(ctx, rx, iq, e); e += 15
    r = _check8(ctx, oracle, c8, t8, max_cand=600, syncmin=1.2)
    assert 200 < len(r["cands"]) == len(r["llr"]) < 600
    # many, then few, in the same buffers
    ctx.enable_sync(True, 1.5, 200, 200, 3000)
    c4 = ctx.channel_open(rx, d4, "FT4")
    iq, _ = S.pair_iq(oracle, 342, [(d8, S.LISTS_MANY8)], [(d4, S.LISTS_MANY4)])
    t8, t4 = _pair(ctx, rx, iq, e); e += 15
    many8 = _check8(ctx, oracle, c8, t8)
    many4 = _check4(ctx, oracle, c4, t4, max_cand=200)
    iq, tones = S.pair_iq(oracle, 343, [(d8, S.LISTS_FEW8)], [(d4, S.LISTS_FEW4)])
    t8, t4 = _pair(ctx, rx, iq, e); e += 15
    few8 = _check8(ctx, oracle, c8, t8)
    few4 = _check4(ctx, oracle, c4, t4, max_cand=200)
    assert 1 <= len(few8["cands"]) < len(many8["cands"]) and 1 <= len(few4["cands"]) < len(many4["cands"]) and 1 <= len(few4["recs"]) < len(many4["recs"])
    S.assert_ft8_found(few8["cands"], few8["llr"], few8["nsync"], S.LISTS_FEW8, tones[("FT8", d8)])
    S.assert_ft4_found(few4["recs"], few4["llr"], few4["nsync"], S.LISTS_FEW4, tones[("FT4", d4)])
    more8 = ctx.fetch_ft8_softbits(c8, len(many8["cands"]) + 50)
    assert more8[0].shape == (len(few8["cands"]), 174) and np.array_equal(more8[0].view(U32), few8["llr"].view(U32))
    more4 = ctx.fetch_ft4_softbits(c4, 3 * len(many4["cands"]) + 50)
    assert more4[0].shape == (len(few4["recs"]), 3, 174) and np.array_equal(more4[0].view(U32), few4["llr"].view(U32))


def test_ft4_refine_and_soft_bits_at_the_band_edges(ctx, oracle):
    """Gap 5 (band): with cwslg_enable_sync(1.5, 100, 100, 5000) getcandidates4 accepts peaks from 200 to 4910 Hz, and ft4_refine_kernel /
    ft4_softbits_kernel (grids (max_cand, 1) and (3 max_cand, 1)) place ft4_downsample's 630-bin window at its lowest and highest positions in the
    36289-bin spectrum.  Bursts with tone 0 at 215 Hz and at 4830 Hz and one mid-band: at least one record has f1_hz < 260 and one f1_hz > 4700;
    candidates, ft4_cd0 of the first candidate, every sync record and every soft record are exact, and the edge bursts decode (nsync 16, the signs
    of set 0 are ft4_softbits_ref.tone_bits of the transmitted tones)."""
    iq, tones = S.build_iq(oracle, 350, N4, ft4=[(S.EDGE_DIAL, S.EDGE_BURSTS)])
    ctx.enable_sync(True, 1.5, 100, 100, 5000)
    ctx.enable_ft4_coherent(True)
    ctx.enable_ft4_softbits(True)
    rx = ctx.receiver_open(FS, BLK, 0)
    ch = ctx.channel_open(rx, S.EDGE_DIAL, "FT4")
    ctx.slot_boundary("FT4", 10)
    _push(ctx, rx, iq)
    ctx.slot_boundary("FT4", 17)
    r = _check4(ctx, oracle, ch, 10, f_lo=100, f_hi=5000)
    cd0, _ = oracle.ft4_downsample(r["cx"], np.float32(r["cands"][0][3]))
    assert np.array_equal(ctx.sync_debug(ch, "ft4_cd0").view(U32), cd0.view(U32))
    assert np.array_equal(ctx.sync_debug(ch, "ft4_cx").view(U32), r["cx"].view(U32))
    f1 = [h["f1_hz"] for h in r["recs"]]
    assert min(f1) < 260 and max(f1) > 4700, (min(f1), max(f1))
    S.assert_ft4_found(r["recs"], r["llr"], r["nsync"], S.EDGE_BURSTS, tones[("FT4", S.EDGE_DIAL)])
    q_lo, q_hi = S.ft4_best(r["recs"], S.EDGE_BURSTS[0]), S.ft4_best(r["recs"], S.EDGE_BURSTS[1])
    assert r["recs"][q_lo]["f1_hz"] < 260 and r["recs"][q_hi]["f1_hz"] > 4700


def test_fetch_slot_agrees_with_the_soft_fetches(xctx, oracle):
    """Gap 6, cwslg_fetch_slot next to the soft-bit fetches: one FT8 and one FT4 channel, both features on.  The one-ticket fetch
    (cwsl_gpu.hip, cwslg_fetch_slot: `out->start_epoch = ch.frame_t0;`, the list only `if (... && channel_records_epoch(ch, REC_CAND, ch.syncbuf.d_block, true))`:
    its stamp is the frame's epoch and not 0) and the separate fetches (cwslg_fetch_ft8_softbits / cwslg_fetch_ft4_softbits: records only while the
    REC_SOFT8 / REC_SOFT4 rule of csrc/record_kinds.hpp holds, own stamp == the list's == frame_t0) agree on
    epoch, list and record order: t_start, list and ft4_sync are equal, and soft record k belongs to list entry / sync record k of THAT ticket --
    three records of each kind are recomputed with the restatement from fetch_slot's own frame and list."""
    ctx = xctx
    ctx.enable_sync(True, 1.5, 100, 200, 3000)
    ctx.enable_ft8_softbits(True)
    ctx.enable_ft4_softbits(True)
    rx = ctx.receiver_open(FS, BLK, 0)
    c8 = ctx.channel_open(rx, S.TICKET_FT8[0][0], "FT8")
    c4 = ctx.channel_open(rx, S.TICKET_FT4[0][0], "FT4")
    iq, tones = S.pair_iq(oracle, 360, S.TICKET_FT8, S.TICKET_FT4)
    _start(ctx, 1)
    t8, t4 = _pair(ctx, rx, iq, 1)
    s8, s4 = ctx.fetch_slot(c8), ctx.fetch_slot(c4)
    assert s8["list_kind"] == "FT8" and s4["list_kind"] == "FT4" and s8["t_start"] == t8 and s4["t_start"] == t4
    llr8, sig8, ns8, e8 = ctx.fetch_ft8_softbits(c8, 600, with_epoch=True)
    llr4, sig4, ns4, nq4, e4 = ctx.fetch_ft4_softbits(c4, 1800, with_epoch=True)
    assert e8 == s8["t_start"] and e4 == s4["t_start"]
    assert _key(s8["list"]) == _key(ctx.fetch_candidates(c8, 600)) and _key(s4["list"]) == _key(ctx.fetch_candidates(c4, 600))
    assert np.array_equal(s8["i16"], ctx.fetch_frame(c8)["i16"]) and np.array_equal(s4["i16"], ctx.fetch_frame(c4)["i16"])
    assert s4["ft4_sync"] == ctx.fetch_ft4_sync(c4) and s8["ft4_sync"] == []
    assert len(llr8) == len(s8["list"]) >= 3 and len(llr4) == len(s4["ft4_sync"]) >= 3
    # the ticket's own frame and list, records 0, 1 and the last
    ref8 = S.ft8_reference(oracle, s8["i16"], s8["list"], 992)
    for q in (0, 1, len(llr8) - 1):
        assert np.array_equal(llr8[q].view(U32), ref8["llr"][q].view(U32)) and sig8[q].view(U32) == ref8["sigma"][q].view(U32) and ns8[q] == ref8["nsync"][q], q
    assert s4["ft4_sync"] == oracle.ft4_sync_all(s4["i16"], s4["list"])
    cx = oracle.ft4_bigspec(s4["i16"])
    pick = [0, 1, len(llr4) - 1]
    rl, rs, rn, rq = R4.softbits_of_records(oracle, cx, [s4["ft4_sync"][q] for q in pick])
    for j, q in enumerate(pick):
        assert np.array_equal(llr4[q].view(U32), rl[j].view(U32)) and np.array_equal(sig4[q].view(U32), rs[j].view(U32)) and ns4[q] == rn[j] and nq4[q] == rq[j], q
    # and the whole of both channels against oracle and restatement, bursts found
    r8, r4 = _check8(ctx, oracle, c8, t8, max_cand=100), _check4(ctx, oracle, c4, t4)
    S.assert_ft8_found(r8["cands"], r8["llr"], r8["nsync"], S.TICKET_FT8[0][1], tones[("FT8", S.TICKET_FT8[0][0])])
    S.assert_ft4_found(r4["recs"], r4["llr"], r4["nsync"], S.TICKET_FT4[0][1], tones[("FT4", S.TICKET_FT4[0][0])])
