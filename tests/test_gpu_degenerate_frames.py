"""GPU: the whole 15 s / 7.5 s chain -- spectra, Costas / candidate search, FT4 refinement, soft bits, BP, OSD, harvest, signal reports -- on the
inputs that are NOT transmissions in noise: digital silence, an impulse, DC, carriers on and off the bin grid, a carrier that starts in mid-slot,
noise-free transmissions, slots whose IQ stops or starts in the middle, a weak station 40 dB under a blocker, a comb of carriers (recipes and
conditions: tests/degenerate_cases.py; tests/test_degenerate_inputs.py proves on the CPU what every recipe puts before the kernels).

One exact-mode context per test, one receiver per recipe with one FT8 and one FT4 channel at dial 0, every feature on: sync, FT4 coherent, FT8
and FT4 soft bits, the code loaded, BP, OSD.  Every test runs three pair slots: the ordinary noisy slot with transmissions on every channel,
the recipes, the ordinary slot again -- nothing of a neighbouring epoch may show in any result and the chain must recover.  The list limits are
200 for the FT8 group and 100 for the FT4 group: cwslg_enable_sync is called before each group's boundary.

Standard of comparison: BIT-EXACT, every record, none skipped, no tolerance.  For every channel of every slot the frame equals the oracle's
(so the CPU-vetted conditions carry over) and every stage equals the restatement applied to the stage before it: the spectra plane, red, red2,
jpeak, jpeak2 over ia..ib and the list (FT8); savsm / sbase, the list, ft4_cx and the sync records (FT4); the soft records (llr and sigma as
uint32, nsync, nqual); the BP and OSD records as bytes.  (degenerate_cases.reference computes the chain once per frame; because every stage is
compared before the next, "the restatement of the GPU's own previous stage" and "the next stage of the chain" are the same array.)  Then per
boundary cwslg_fetch_decodes of both groups against decodes_ref on the GPU's own records, cwslg_fetch_decode_reports against
decode_reports_ref on the GPU's own planes and lists, and cwslg_fetch_ft4_decode_reports against ft4_decode_reports_ref on the GPU's own frame
spectra (ft4_cx) and sync records, its nsync against the soft records' (first-half epochs included; test_degenerate_inputs.py lists the FT4
decodes the recipes give: records with ibest < 0, OSD-only words, noise-free transmissions).
One allowance, from tests/test_gpu_longsync_edges.py: the FT4 baseline (`red2`) of an
all-zero frame is NaN in the restatement (degenerate_cases.NAN_ALLOWED); there the GPU's value must be a NaN too, of any payload.

The FT4 channel's frame of a pair slot is its second half, for `midslot` its first half as well (the all-zero one); the first half of the other
recipes takes part in the FT4 group fetch of its epoch with the GPU's own records, its chain is not restated a second time.  With open gates and
OSD order 2 the numpy OSD is the host's largest cost (about 3 s per 200 records on one core); measured through the CPU module on one core the
host side of a case is at most 12 s (carriers, open gates) to 15 s (cut, open gates), which does not exceed the limit this module was given
(about 15 s), so the list limits are 200 / 100 in both configurations, OSD runs included.

Wall times on an MI355X, seconds per test (call phase), in the run of the whole GPU suite that first held this module (642 passed in 365 s), the
ordinary slot's chain computed once per configuration and shared; in brackets each case alone in a process of its own:
    quiet-upstream 2.2 (2.3)    carriers-upstream 2.3 (3.6)    clean-upstream < 2.0 (2.6)    cut-upstream < 2.0 (2.8)
    quiet-open     5.1 (5.8)    carriers-open     3.5 (7.5)    clean-open       3.8 (6.1)    cut-open       4.9 (7.8)
The yardstick, tests/test_gpu_softbits_scale.py in the same run: 2.7 s (both features), 2.2 s (reconfigure), 2.0 s (open and close), the others
below 2 s; twice the slowest is 5.3 s, so no case is split.

test_fast_mode_chain runs the groups `clean` and `cut` under UPSTREAM once more after cwslg_set_exact(ctx, 0): the frame within 1 LSB of the
oracle's at every sample (all zero where the oracle's is; on an MI355X 35 and 34 of the 36 frames of a run are not the oracle's, 5873 and 2673
samples in all), everything behind it as above, on the fast mode's own frames.  One condition of
assert_conditions is not asserted there (degenerate_cases.assert_conditions says which and why).  With the FT4 report calls in, on an MI355X
in a run of this module after tests/test_gpu_record_fetch_races.py: clean-upstream 1.7, cut-upstream 1.6, clean-open 3.8, cut-open 4.8,
quiet-open 5.0, fast-clean 2.0, fast-cut 1.3 s."""
import numpy as np
import pytest

import decode_reports_ref as RR
import decodes_ref as DR
import degenerate_cases as G
import ft4_decode_cases as D
import ft4_decode_reports_ref as R4
import ldpc_cases as LC

pytestmark = pytest.mark.gpu
FS, BLK, N4, N8 = G.FS, G.BLK, G.N4, G.N8
U32 = np.uint32
BIG = 1 << 16


@pytest.fixture
def xctx():
    """A fresh context in the default (exact) arithmetic mode: the frames are the oracle's, bit for bit."""
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


def _push(ctx, rx, iq):
    iq = np.ascontiguousarray(iq, dtype=np.complex64)
    for k in range(0, len(iq), 64 * BLK):
        ctx.push_iq(rx, iq[k:k + 64 * BLK])


def _sync(ctx, mode):
    ctx.enable_sync(True, G.SYNCMIN8, G.MAX_CAND[mode], G.F_LO, G.F_HI)


def _configure(ctx, cfg):
    _sync(ctx, "FT8")
    ctx.set_ft4_syncmin(G.SYNCMIN4)
    ctx.enable_ft4_coherent(True)
    ctx.set_ldpc_code(LC.make_code(G.SEED)["nm"])
    ctx.enable_ft8_softbits(True)
    ctx.enable_ft4_softbits(True)
    ctx.enable_ft8_decode(True, cfg.max_iter, cfg.min_nsync8)
    ctx.enable_ft4_decode(True, cfg.max_iter, cfg.min_nsync4, cfg.min_nqual4)
    ctx.enable_ft8_osd(True, cfg.order, cfg.min_nsync8)
    ctx.enable_ft4_osd(True, cfg.order, cfg.min_nsync4, cfg.min_nqual4)


def _boundary(ctx, mode, epoch):
    _sync(ctx, mode)                                                    # the group's own list limit, in force at its boundary
    ctx.slot_boundary(mode, epoch)


def _key(cands):
    return [(c[0], c[1]) + tuple(int(np.float32(x).view(U32)) for x in c[2:]) for c in cands]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(U32)


FAST_FRAMES = []                                                        # fast mode: (samples 1 LSB off the oracle's, samples) per frame compared


def _frame(ctx, ch, t_start, want_frame, exact):
    """The channel's frame of epoch t_start.  Exact mode: the oracle's, bit for bit.  Fast mode: within 1 LSB of the oracle's at every sample, and
    all zero where the oracle's frame is all zero."""
    fr = ctx.fetch_frame(ch)
    assert fr is not None and fr["t_start"] == t_start, (ch, fr and fr["t_start"], t_start)
    if exact:
        assert np.array_equal(fr["i16"], want_frame), (ch, t_start)
    else:
        assert fr["i16"].shape == want_frame.shape and fr["i16"].dtype == np.int16
        off = np.abs(fr["i16"].astype(np.int32) - want_frame.astype(np.int32))
        assert off.max() <= 1 and (want_frame.any() or not fr["i16"].any()), (ch, t_start, int(off.max()))
        FAST_FRAMES.append((int(np.count_nonzero(off)), off.size))
    return fr


def _check8(ctx, oracle, ch, t_start, want_frame, cfg, exact=True):
    """One FT8 channel, one epoch: every stage against the restatement.  -> the GPU's outputs arranged like degenerate_cases.reference's."""
    fr = _frame(ctx, ch, t_start, want_frame, exact)
    ref = G.reference(oracle, "FT8", fr["i16"], cfg)
    plane = ctx.sync_debug(ch, "spectra")
    assert plane.shape == (372, G.PITCH) and np.array_equal(_bits(plane), _bits(ref["plane"])), (ch, plane.shape)
    arrays = {}
    for name in ("red", "red2", "jpeak", "jpeak2"):
        arrays[name] = ctx.sync_debug(ch, name).copy()
        got, want = arrays[name][G.IA:G.IB + 1], ref["arrays"][name][G.IA:G.IB + 1]
        assert np.array_equal(got.view(U32), want.view(U32)), (ch, name, np.nonzero(got.view(U32) != want.view(U32))[0][:5])
    cands, t_c = ctx.fetch_candidates(ch, 600, with_epoch=True)
    assert t_c == t_start and _key(cands) == _key(ref["list"]), (ch, t_c, len(cands), len(ref["list"]))
    soft = ctx.fetch_ft8_softbits(ch, 600, with_epoch=True)
    msg = ctx.fetch_ft8_decode(ch, 600, with_epoch=True)
    osd = ctx.fetch_ft8_osd(ch, 600, with_epoch=True)
    assert soft is not None and msg is not None and osd is not None, (ch, soft is None, msg is None, osd is None)
    llr, sigma, nsync, t_s = soft
    assert t_s == msg[1] == osd[1] == t_start and len(llr) == len(msg[0]) == len(osd[0]) == len(cands)
    bad = np.nonzero((_bits(llr) != _bits(ref["llr"])).any(axis=1) | (_bits(sigma) != _bits(ref["sigma"])) | (nsync != ref["nsync"]))[0]
    assert bad.size == 0, ("soft", ch, bad[:5], [cands[q][:2] for q in bad[:5]])
    for kind, got, want in (("msg", msg[0], ref["msg"]), ("osd", osd[0], ref["osd"])):
        assert got.dtype.itemsize == want.dtype.itemsize
        bad = [q for q in range(len(want)) if got[q].tobytes() != want[q].tobytes()]
        assert not bad, (kind, ch, bad[:5], got[bad[:2]], want[bad[:2]])
    return dict(frame=fr["i16"], plane=plane, arrays=arrays, list=cands, llr=llr, sigma=sigma, nsync=nsync, msg=msg[0], osd=osd[0])


def _check4(ctx, oracle, ch, t_start, want_frame, cfg, nan_ok=False, exact=True):
    """One FT4 channel, one epoch: every stage against the restatement."""
    fr = _frame(ctx, ch, t_start, want_frame, exact)
    ref = G.reference(oracle, "FT4", fr["i16"], cfg)
    arrays = dict(savsm=ctx.sync_debug(ch, "red")[:1153].copy(), sbase=ctx.sync_debug(ch, "red2")[:1153].copy())
    for name in ("savsm", "sbase"):
        want = ref["arrays"][name]
        assert nan_ok or not np.isnan(want).any(), (ch, name)
        assert G.same_bits(arrays[name], want), (ch, name, arrays[name][36:42], want[36:42])
    cands, t_c = ctx.fetch_candidates(ch, 600, with_epoch=True)
    assert t_c == t_start and _key(cands) == _key(ref["list"]), (ch, t_c, len(cands), len(ref["list"]))
    cx = ctx.sync_debug(ch, "ft4_cx")
    assert np.array_equal(cx.view(U32), ref["cx"].view(U32)), ch
    recs = ctx.fetch_ft4_sync(ch, 1800, with_epoch=True)
    soft = ctx.fetch_ft4_softbits(ch, 1800, with_epoch=True)
    msg = ctx.fetch_ft4_decode(ch, 1800, with_epoch=True)
    osd = ctx.fetch_ft4_osd(ch, 1800, with_epoch=True)
    assert recs is not None and soft is not None and msg is not None and osd is not None, (ch, recs is None, soft is None, msg is None, osd is None)
    llr, sigma, nsync, nqual, t_s = soft
    assert recs[1] == t_s == msg[1] == osd[1] == t_start
    assert recs[0] == ref["recs"], (ch, len(recs[0]), len(ref["recs"]))
    assert len(llr) == len(msg[0]) == len(osd[0]) == len(recs[0]) and llr.shape == ref["llr"].shape and sigma.shape == ref["sigma"].shape
    bad = np.nonzero((_bits(llr) != _bits(ref["llr"])).any(axis=(1, 2)) | (_bits(sigma) != _bits(ref["sigma"])).any(axis=1)
                     | (nsync != ref["nsync"]) | (nqual != ref["nqual"]))[0]
    assert bad.size == 0, ("soft", ch, bad[:5], [recs[0][q] for q in bad[:3]])
    for kind, got, want in (("msg", msg[0], ref["msg"]), ("osd", osd[0], ref["osd"])):
        assert got.dtype.itemsize == want.dtype.itemsize
        bad = [q for q in range(len(want)) if got[q].tobytes() != want[q].tobytes()]
        assert not bad, (kind, ch, bad[:5], got[bad[:2]], want[bad[:2]])
    return dict(frame=fr["i16"], arrays=arrays, list=cands, cx=cx, recs=recs[0], llr=llr, sigma=sigma, nsync=nsync, nqual=nqual,
                msg=msg[0].view(D.MSG4_DTYPE).reshape(-1), osd=osd[0].view(G.X.OSD4_DTYPE).reshape(-1))


def _own4(ctx, ch, t_start, want_frame, exact=True):
    """The frame and the GPU's own records of an FT4 channel, for the group fetches alone: the first half of a recipe whose FT4 frame is the
    second half is more of the same signal, and its chain is not restated a second time.  The frame spectrum and the soft records' nsync come
    along for the reports."""
    _frame(ctx, ch, t_start, want_frame, exact)
    recs, soft, msg, osd = (f(ch, 1800, with_epoch=True) for f in (ctx.fetch_ft4_sync, ctx.fetch_ft4_softbits, ctx.fetch_ft4_decode, ctx.fetch_ft4_osd))
    assert recs is not None and soft is not None and msg is not None and osd is not None and recs[1] == soft[-1] == msg[1] == osd[1] == t_start
    assert len(recs[0]) == len(soft[2]) == len(msg[0]) == len(osd[0])
    return dict(recs=recs[0], cx=ctx.sync_debug(ch, "ft4_cx"), nsync=soft[2], msg=msg[0].view(D.MSG4_DTYPE).reshape(-1),
                osd=osd[0].view(G.X.OSD4_DTYPE).reshape(-1))


def _group_fetch(ctx, mode, E, got_by_ch):
    """cwslg_fetch_decodes and the mode's report fetch (cwslg_fetch_decode_reports / cwslg_fetch_ft4_decode_reports) of epoch E against the
    restatements on the GPU's own records, planes (FT8) and frame spectra (FT4) of the channels in got_by_ch {ch_id: outputs of _check8 /
    _check4 / _own4}, which must be the channels that take part.  -> the decodes."""
    want, total = DR.decodes(mode, [G.decodes_of(mode, ch, g) for ch, g in got_by_ch.items()])
    for ask in (0, E):
        r = ctx.fetch_decodes(mode, ask, BIG)
        assert r is not None, (mode, E)
        dec, E_got, n_total, n_ch = r
        assert (E_got, n_total, n_ch) == (E, total, len(got_by_ch)), (mode, ask, E_got, n_total, n_ch, total, len(got_by_ch))
        assert dec.dtype == DR.DECODE_DTYPE and dec.tobytes() == want.tobytes(), (mode, dec[:3], want[:3])
    if mode == "FT8":
        dec2, rep, E_got, n_total, n_ch = ctx.fetch_decode_reports("FT8", E, BIG)
        assert (E_got, n_total, n_ch) == (E, total, len(got_by_ch)) and dec2.tobytes() == want.tobytes() and rep.dtype == RR.REPORT_DTYPE
        chans = sorted({int(c) for c in want["ch_id"]})
        want_rep = G.reports_of({ch: got_by_ch[ch]["plane"] for ch in chans}, {ch: got_by_ch[ch]["list"] for ch in chans}, want)
    else:
        dec2, rep, E_got, n_total, n_ch = ctx.fetch_ft4_decode_reports(E, BIG)
        assert (E_got, n_total, n_ch) == (E, total, len(got_by_ch)) and dec2.tobytes() == want.tobytes() and rep.dtype == R4.REPORT_DTYPE
        chans = sorted({int(c) for c in want["ch_id"]})
        want_rep = G.reports4_of({ch: got_by_ch[ch]["cx"] for ch in chans}, {ch: got_by_ch[ch]["recs"] for ch in chans}, want)
    bad = [p for p in range(len(want)) if rep[p].tobytes() != want_rep[p].tobytes()]
    assert not bad, (mode, bad[:5], rep[bad[:3]], want_rep[bad[:3]], want[bad[:3]])
    for ch in chans:                                                    # the report's nsync is the soft record's
        sel = want["ch_id"] == ch
        assert np.array_equal(rep["nsync"][sel], np.asarray(got_by_ch[ch]["nsync"])[want["entry"][sel]])
    return want


def _assert_empty(ctx, mode, ch, t_start):
    """Every list and record fetch of a zero-frame channel's epoch hands out nothing, under that epoch."""
    cands, t_c = ctx.fetch_candidates(ch, 600, with_epoch=True)
    assert (cands, t_c) == ([], t_start)
    if mode == "FT8":
        fetches = (ctx.fetch_ft8_softbits, ctx.fetch_ft8_decode, ctx.fetch_ft8_osd)
    else:
        fetches = (ctx.fetch_ft4_sync, ctx.fetch_ft4_softbits, ctx.fetch_ft4_decode, ctx.fetch_ft4_osd)
    for f in fetches:
        r = f(ch, 600, with_epoch=True)
        assert r is not None and r[-1] == t_start and len(r[0]) == 0, (mode, ch, f.__name__, r)


def _run(ctx, oracle, group, cfg, exact=True):
    names = G.GROUPS[group]
    _configure(ctx, cfg)
    rxs = [ctx.receiver_open(FS, BLK, 0) for _ in names]
    c8 = [ctx.channel_open(rx, G.DIAL, "FT8") for rx in rxs]
    c4 = [ctx.channel_open(rx, G.DIAL, "FT4") for rx in rxs]
    ordinary_iq, tones = G.ordinary()
    ord_first_half = G.oracle_frame(oracle, "FT4", ordinary_iq, 0)
    e = 1
    _boundary(ctx, "FT8", e)
    _boundary(ctx, "FT4", e)
    counts = {}
    for slot in range(3):
        recipe_slot = slot == 1
        iqs = [G.recipe_iq(n) for n in names] if recipe_slot else [ordinary_iq] * len(names)
        for rx, iq in zip(rxs, iqs):
            _push(ctx, rx, iq[:N4])
        _boundary(ctx, "FT4", e + 8)
        # the FT4 group's first-half epoch: compared where a recipe names it (midslot: the all-zero frame); the group fetch on all its channels
        first = {}
        for k, n in enumerate(names):
            if recipe_slot and G.RECIPES[n] == 0:
                first[c4[k]] = _check4(ctx, oracle, c4[k], e, G.recipe_frame(n, "FT4"), cfg, nan_ok=(n, "FT4") in G.ZERO_FRAMES, exact=exact)
                G.assert_conditions(n, "FT4", cfg, first[c4[k]], fast_frame=not exact)
                if (n, "FT4") in G.ZERO_FRAMES:
                    _assert_empty(ctx, "FT4", c4[k], e)
                counts[(n, "FT4")] = (len(first[c4[k]]["list"]), len(first[c4[k]]["recs"]))
            elif recipe_slot:
                first[c4[k]] = _own4(ctx, c4[k], e, G.oracle_frame(oracle, "FT4", G.recipe_iq(n), 0), exact=exact)
            else:
                first[c4[k]] = _check4(ctx, oracle, c4[k], e, ord_first_half, cfg, exact=exact)
        dec = _group_fetch(ctx, "FT4", e, first)
        if recipe_slot:
            zero = {c4[k] for k, n in enumerate(names) if G.RECIPES[n] == 0 and (n, "FT4") in G.ZERO_FRAMES}
            assert not zero & {int(c) for c in dec["ch_id"]}
        for rx, iq in zip(rxs, iqs):
            _push(ctx, rx, iq[N4:])
        _boundary(ctx, "FT8", e + 15)
        _boundary(ctx, "FT4", e + 15)
        got8, got4 = {}, {}
        for k, n in enumerate(names):
            want8 = G.recipe_frame(n, "FT8") if recipe_slot else G.ordinary_frame("FT8")
            want4 = (G.recipe_frame(n, "FT4") if G.RECIPES[n] == 1 else G.oracle_frame(oracle, "FT4", G.recipe_iq(n), 1)) if recipe_slot else G.ordinary_frame("FT4")
            got8[c8[k]] = _check8(ctx, oracle, c8[k], e, want8, cfg, exact=exact)
            got4[c4[k]] = _check4(ctx, oracle, c4[k], e + 8, want4, cfg, nan_ok=not want4.any(), exact=exact)
            if recipe_slot:
                G.assert_conditions(n, "FT8", cfg, got8[c8[k]], fast_frame=not exact)
                counts[(n, "FT8")] = (len(got8[c8[k]]["list"]),)
                if n == "blocker8" and not exact:
                    print(f"\n[degenerate frames] fast mode, blocker8 FT8: max |llr| {np.abs(got8[c8[k]]['llr']).max():.1f} (the condition dropped for fast mode asks for 1000)")
                if G.RECIPES[n] == 1:
                    G.assert_conditions(n, "FT4", cfg, got4[c4[k]], fast_frame=not exact)
                    counts[(n, "FT4")] = (len(got4[c4[k]]["list"]), len(got4[c4[k]]["recs"]))
                for mode, ch, t in (("FT8", c8[k], e), ("FT4", c4[k], e + 8)):
                    if (n, mode) in G.ZERO_FRAMES and not (mode == "FT4" and G.RECIPES[n] == 0):
                        _assert_empty(ctx, mode, ch, t)
            else:
                G.assert_ordinary("FT8", got8[c8[k]], tones)
                G.assert_ordinary("FT4", got4[c4[k]], tones)
        dec8 = _group_fetch(ctx, "FT8", e, got8)
        dec4 = _group_fetch(ctx, "FT4", e + 8, got4)
        if recipe_slot:
            for k, n in enumerate(names):
                if (n, "FT8") in G.ZERO_FRAMES:
                    assert c8[k] not in {int(c) for c in dec8["ch_id"]}
                if (n, "FT4") in G.ZERO_FRAMES and G.RECIPES[n] == 1:
                    assert c4[k] not in {int(c) for c in dec4["ch_id"]}
        e += 15
    print(f"\n[degenerate frames] {group} / {cfg.name}{'' if exact else ' / fast mode'}: (list[, records]) compared per recipe: " + ", ".join(f"{n} {m} {c}" for (n, m), c in sorted(counts.items())))


@pytest.mark.parametrize("cfg", [G.UPSTREAM, G.OPEN], ids=lambda c: c.name)
@pytest.mark.parametrize("group", list(G.GROUPS))
def test_degenerate_frames(xctx, oracle, group, cfg):
    _run(xctx, oracle, group, cfg)


@pytest.mark.parametrize("group", ["clean", "cut"])
def test_fast_mode_chain(xctx, oracle, group):
    """The same run after cwslg_set_exact(ctx, 0): BP, OSD, the harvest and both report kernels on the fast mode's frames.  Only the frame's
    assertion changes (within 1 LSB of the oracle's, all zero where the oracle's is); every later stage is compared on bits with the
    restatement of the GPU's own previous stage, the group fetches and both report fetches as in exact mode, and assert_conditions runs on the
    GPU's outputs."""
    xctx.set_exact(False)
    del FAST_FRAMES[:]
    _run(xctx, oracle, group, G.UPSTREAM, exact=False)
    moved = [m for m, _ in FAST_FRAMES if m]
    print(f"[degenerate frames] fast mode: {len(FAST_FRAMES)} frames compared, {len(moved)} of them not the oracle's, {sum(moved)} samples 1 LSB off")
    assert moved                                                        # (the run did use the other arithmetic)
