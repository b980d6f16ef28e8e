"""GPU: the FT4 decode (cwslg_ft4_msg) through the C ABI at 48 kHz.  PARITY UNPINNED by the reference; every comparison is BYTE EQUALITY of whole
60-byte records against tests/ft4_decode_cases.py:expected() -- the numpy restatement of cwslg_ft8_msg (tests/ldpc_ref.py) per metric set with the
two gates -- applied to the GPU's own fetched cwslg_ft4_soft records.  No tolerance anywhere.  The inputs are vetted on the CPU in
tests/test_ft4_decode_inputs.py; as stated there, no recipe reaches sigma[s] == 0."""
import numpy as np
import pytest

import ft4_decode_cases as D
import ldpc_cases as C
import ldpc_ref as R

pytestmark = pytest.mark.gpu
FS, BLK, N4 = D.FS, D.BLK, D.N4
U32 = np.uint32
ARG, MODE = -6, -5
UPSTREAM = (30, 8, 20)


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


def _sync(ctx, max_cand, syncmin4=D.SYNCMIN_FT4):
    ctx.enable_sync(True, D.SYNC["syncmin"], max_cand, D.SYNC["f_lo"], D.SYNC["f_hi"])
    ctx.set_ft4_syncmin(syncmin4)                                      # (cwslg_enable_sync starts from the default threshold)


def _open(ctx, seed, max_cand, rfs, syncmin4=D.SYNCMIN_FT4, decode=UPSTREAM):
    """Sync stage, FT4 soft bits, the seed's code and (decode not None) the decode; one receiver, FT4 channels at rfs, the first frame begun."""
    _sync(ctx, max_cand, syncmin4)
    ctx.enable_ft4_softbits(True)
    ctx.set_ldpc_code(C.make_code(seed)["nm"])
    if decode:
        ctx.enable_ft4_decode(True, *decode)
    rx = ctx.receiver_open(FS, BLK, 0)
    chans = [ctx.channel_open(rx, rf, "FT4") for rf in rfs]
    ctx.slot_boundary("FT4", 10)
    return rx, chans


class _Slots:
    """Consecutive FT4 slots of one receiver: run(iq) pushes a slot and closes it; t is the start epoch of the frame just finalised."""

    def __init__(self, ctx, rx):
        self.ctx, self.rx, self.epoch, self.t = ctx, rx, 10, None

    def run(self, iq):
        before = self.ctx.stats()["sync_launches"]
        _push(self.ctx, self.rx, iq)
        self.t = self.epoch
        self.epoch += 7
        self.ctx.slot_boundary("FT4", self.epoch)
        self.ctx.synchronize()
        return self.ctx.stats()["sync_launches"] - before


def _same(got, want):
    assert got.dtype == want.dtype == D.MSG4_DTYPE and got.shape == want.shape, (got.shape, want.shape)
    bad = [q for q in range(len(want)) if got[q].tobytes() != want[q].tobytes()]
    assert not bad, (bad[:5], [(got[q], want[q]) for q in bad[:3]])


def _check(ctx, ch, code, params, t=None, max_cand=D.MAX_CAND):
    """Decode records, soft records, sync records, list and frame of one epoch; every decode record is expected() of the GPU's own soft record."""
    fr = ctx.fetch_frame(ch)
    cands, t_c = ctx.fetch_candidates(ch, max_cand, with_epoch=True)
    recs = ctx.fetch_ft4_sync(ch)
    llr, sigma, nsync, nqual, t_s = ctx.fetch_ft4_softbits(ch, with_epoch=True)
    got = ctx.fetch_ft4_decode(ch, with_epoch=True)
    assert got is not None, "no decode records of the current epoch"
    rec, t_m = got
    assert t_m == t_s == t_c == fr["t_start"] and (t is None or t_m == t), (t_m, t_s, t_c, fr["t_start"], t)
    assert len(rec) == len(recs) == len(llr)
    soft = D.soft_dict(llr, sigma, nsync, nqual)
    _same(rec, D.expected(soft, code, *params))
    return dict(rec=rec, soft=soft, recs=recs, cands=cands, fr=fr)


def _na(rec):
    """Which records are the not-attempted pattern in all three sets, checked field by field."""
    s = rec["set"]
    na = (s["iters"] == -1).all(axis=1)
    assert ((s["iters"] == -1) == (s["nbad"] == -1)).all() and ((s["iters"] == -1) == (s["nharderr"] == -1)).all()
    assert not s["bits"][s["iters"] == -1].any() and not s["crc_ok"][s["iters"] == -1].any() and not s["pad_"].any()
    return na


def test_chain_ft4_and_ft8_decode_side_by_side(xctx):
    """Two FT4 channels whose transmissions carry codewords and one FT8 channel with the FT8 decode on, in one context on one stretch of IQ: the FT4
    boundary and the FT8 boundary queue the kernel in both addressing modes back to back.  Every FT4 record matches, every message sent comes
    out under ft4_best_set, the FT8 records still equal the restatement, and the decode fetch's epoch is the sync fetch's."""
    from cwsl_digi_amd.api import ft4_best_set
    ctx = xctx
    seed = C.SEEDS[0]
    code = C.make_code(seed)["code"]
    chans4 = D.RECIPES["chain"][2]
    iq = np.array(C.chain_iq(seed))
    iq[-N4:] = D.recipe_iq("chain", seed)                              # (the recipe is that tail plus the FT4 transmissions)
    _sync(ctx, D.MAX_CAND)
    ctx.enable_ft4_softbits(True)
    ctx.enable_ft8_softbits(True)
    ctx.set_ldpc_code(C.make_code(seed)["nm"])
    ctx.enable_ft4_decode(True, *UPSTREAM)
    ctx.enable_ft8_decode(True, 30, 7)
    rx = ctx.receiver_open(FS, BLK, 0)
    c4 = [ctx.channel_open(rx, rf, "FT4") for rf, _ in chans4]
    c8 = ctx.channel_open(rx, D.FT8_CHAIN[0], "FT8")
    ctx.slot_boundary("FT8", 1)
    _push(ctx, rx, iq[:-N4])
    ctx.slot_boundary("FT4", 10)
    _push(ctx, rx, iq[-N4:])
    ctx.slot_boundary("FT4", 17)
    ctx.slot_boundary("FT8", 16)
    for ch, (rf, txs) in zip(c4, chans4):
        r = _check(ctx, ch, code, UPSTREAM, t=10)
        na = _na(r["rec"])
        assert na.any() and not na.all() and (na == ((r["soft"]["nsync"] < 8) | (r["soft"]["nqual"] < 20))).all()
        best = ft4_best_set(r["rec"])
        assert np.array_equal(best, D.best_set(r["rec"]))
        for audio, t0, amp, mseed in txs:
            qs = D.find_message(r["rec"], D.message(mseed))
            assert qs and abs(r["recs"][qs[0]]["f1_hz"] - audio) <= 3.0, (rf, audio)
            assert ft4_best_set(r["rec"][qs[0]]) == best[qs[0]] >= 0
    # a caller's own smaller `max` cuts the records like the sync records
    two = ctx.fetch_ft4_decode(c4[0], 2)
    assert len(two) == 2 and two.tobytes() == ctx.fetch_ft4_decode(c4[0])[:2].tobytes()
    # the FT8 form beside it
    cands, t_c = ctx.fetch_candidates(c8, 200, with_epoch=True)
    llr, sigma, nsync, t_s = ctx.fetch_ft8_softbits(c8, 200, with_epoch=True)
    rec8, t_m = ctx.fetch_ft8_decode(c8, 200, with_epoch=True)
    assert t_m == t_s == t_c == 1 and len(rec8) == len(cands) > 5
    want8 = R.hard_records(code, llr, 30, nsync, sigma, 7)
    assert rec8.tobytes() == want8.tobytes() and rec8["crc_ok"].any() and (rec8["iters"] == -1).any()
    from cwsl_digi_amd.api import CwslGpuError
    for fn, ch in ((ctx.fetch_ft4_decode, c8), (ctx.fetch_ft8_decode, c4[0])):
        with pytest.raises(CwslGpuError) as e:
            fn(ch)
        assert e.value.status == MODE


@pytest.mark.parametrize("max_cand", [1, 2, 5])
def test_smallest_shapes_cut_lists_and_holes(xctx, max_cand):
    """9, 18 and 45 waves per channel: the last workgroup is partly empty.  The lists are longer than max_cand and are cut; at 5 the candidates
    have one, two and three records, so the slot array has holes (a candidate with none: the next test)."""
    seed = C.SEEDS[0]
    rfs = [rf for rf, _ in D.RECIPES["small"][2]]
    rx, chans = _open(xctx, seed, max_cand, rfs)
    _Slots(xctx, rx).run(D.recipe_iq("small", seed))
    counts = set()
    for ch in chans:
        r = _check(xctx, ch, C.make_code(seed)["code"], UPSTREAM, t=10, max_cand=max_cand)
        assert len(r["cands"]) == max_cand and len(r["rec"]) >= max_cand
        counts |= set(np.bincount([h["cand"] for h in r["recs"]], minlength=max_cand).tolist())
        _na(r["rec"])
    assert counts == ({1, 2, 3} if max_cand == 5 else {1, 3} if max_cand == 2 else {1}), counts


def test_candidates_with_zero_one_two_and_three_records(xctx):
    """The "carriers" frame at max_cand 17 (153 waves, the last workgroup partly empty, the list cut): its candidates have 0, 1, 2 and 3 records,
    so a wholly empty candidate lies between occupied ones in the slot array -- its nine waves leave, and the fetch's walk skips it, keeping
    record q with entry q of the sync fetch.  Once with upstream's gates and once with every record attempted."""
    seed = C.SEEDS[0]
    code = C.make_code(seed)["code"]
    (rf, _), = D.RECIPES["carriers"][2]
    mc = D.HOLES_MAX_CAND
    rx, (ch,) = _open(xctx, seed, mc, [rf])
    slots = _Slots(xctx, rx)
    for params in (UPSTREAM, (30, 0, 0)):
        xctx.enable_ft4_decode(True, *params)
        slots.run(D.recipe_iq("carriers", seed))
        r = _check(xctx, ch, code, params, t=slots.t, max_cand=mc)
        nrec = np.bincount([h["cand"] for h in r["recs"]], minlength=mc)
        assert len(r["cands"]) == mc and set(nrec.tolist()) == {0, 1, 2, 3}, nrec
        hole = int(np.nonzero(nrec == 0)[0][0])
        assert 0 < hole < mc - 1 and nrec[hole + 1:].sum() > 0 and len(r["rec"]) == nrec.sum()
        if params == (30, 0, 0):
            assert not _na(r["rec"]).any()


def test_noise_only_channel_has_zero_records(xctx):
    seed = C.SEEDS[0]
    (rf_tx, _), (rf_noise, _) = D.RECIPES["small"][2]
    rx, (a, b) = _open(xctx, seed, 2, [rf_tx, rf_noise], syncmin4=D.SYNCMIN_QUIET)
    _Slots(xctx, rx).run(D.recipe_iq("small", seed))
    assert len(_check(xctx, a, C.make_code(seed)["code"], UPSTREAM, t=10, max_cand=2)["rec"]) >= 1
    assert xctx.fetch_candidates(b, 2) == [] and xctx.fetch_ft4_sync(b) == []
    rec, t_m = xctx.fetch_ft4_decode(b, with_epoch=True)               # n == 0, no error
    assert rec.shape == (0,) and rec.dtype == D.MSG4_DTYPE and t_m == 10


def test_gates_and_max_iter(xctx):
    """One channel, the same slot of IQ under six settings (each applies from the next boundary on)."""
    ctx = xctx
    seed = C.SEEDS[0]
    code = C.make_code(seed)["code"]
    rf = D.RECIPES["chain"][2][0][0]
    iq = D.recipe_iq("chain", seed)
    rx, (ch,) = _open(ctx, seed, D.MAX_CAND, [rf], decode=None)
    slots = _Slots(ctx, rx)
    seen = {}
    for params in ((30, 0, 0), (30, 17, 0), (30, 0, 33), (30, 8, 20), (5, 8, 20), (5, 0, 0)):
        ctx.enable_ft4_decode(True, *params)
        slots.run(iq)
        r = _check(ctx, ch, code, params, t=slots.t)
        na = _na(r["rec"])
        assert len(r["rec"]) > 20
        if params[1:] == (0, 0):
            assert not na.any() and (r["soft"]["sigma"] != 0).all() and (r["rec"]["set"]["iters"] >= 0).all()
        elif params[1:] in ((17, 0), (0, 33)):
            assert na.all()
        else:
            assert na.any() and not na.all()                           # both kinds present
        assert r["rec"]["set"]["iters"].max() <= params[0]
        seen[params] = r["rec"]
    assert seen[(5, 8, 20)]["set"]["iters"].max() == 5 and seen[(30, 8, 20)]["set"]["iters"].max() > 5
    assert seen[(5, 8, 20)].tobytes() != seen[(30, 8, 20)].tobytes()


def test_off_means_off(xctx):
    """Decode never enabled: the launches a boundary had, nothing to fetch.  On: one launch more.  Off again, soft bits off, coherent stage off:
    the first slot's launches and nothing to fetch -- never the previous slot's records.  Frames, lists, sync and soft records do not depend on it."""
    ctx = xctx
    seed = C.SEEDS[0]
    code = C.make_code(seed)["code"]
    rf = D.RECIPES["chain"][2][1][0]
    iq = D.recipe_iq("chain", seed)
    rx, (ch,) = _open(ctx, seed, D.MAX_CAND, [rf], decode=None)
    slots = _Slots(ctx, rx)

    def state():
        soft = ctx.fetch_ft4_softbits(ch)
        cands = [tuple(np.float32(x).view(U32) if isinstance(x, float) else x for x in c) for c in ctx.fetch_candidates(ch, D.MAX_CAND)]
        return ctx.fetch_frame(ch)["i16"].tobytes(), cands, ctx.fetch_ft4_sync(ch), None if soft is None else tuple(x.tobytes() for x in soft)

    off = slots.run(iq)
    assert off == 1 and ctx.fetch_ft4_decode(ch) is None
    plain = state()
    assert plain[3] is not None and len(plain[2]) > 20
    ctx.enable_ft4_decode(True, *UPSTREAM)
    assert ctx.fetch_ft4_decode(ch) is None                            # enabling computes nothing by itself: from the next boundary on
    assert slots.run(iq) == off + 1
    assert state() == plain
    rec = _check(ctx, ch, code, UPSTREAM, t=slots.t)["rec"]
    ctx.enable_ft4_decode(False)
    assert slots.run(iq) == off
    assert ctx.fetch_ft4_decode(ch) is None and state() == plain       # not the previous slot's records under this epoch
    ctx.enable_ft4_decode(True, *UPSTREAM)
    assert ctx.fetch_ft4_decode(ch) is None
    assert slots.run(iq) == off + 1
    assert _check(ctx, ch, code, UPSTREAM, t=slots.t)["rec"].tobytes() == rec.tobytes()
    ctx.enable_ft4_softbits(False)                                     # soft bits off at a boundary, the decode still enabled
    assert slots.run(iq) == off
    assert ctx.fetch_ft4_decode(ch) is None and ctx.fetch_ft4_softbits(ch) is None and state()[:3] == plain[:3]
    ctx.enable_ft4_softbits(True)
    assert slots.run(iq) == off + 1
    assert _check(ctx, ch, code, UPSTREAM, t=slots.t)["rec"].tobytes() == rec.tobytes()
    ctx.enable_ft4_coherent(False)                                     # coherent stage off: no records of any kind
    assert slots.run(iq) == off
    assert ctx.fetch_ft4_decode(ch) is None and ctx.fetch_ft4_softbits(ch) is None
    assert ctx.fetch_candidates(ch, D.MAX_CAND, with_epoch=True)[1] == slots.t


def test_life_cycle_reallocation_channels_and_a_second_code(xctx):
    ctx = xctx
    a, b = C.SEEDS
    code_a, code_b = C.make_code(a)["code"], C.make_code(b)["code"]
    (rf0, _), (rf1, _) = D.RECIPES["chain"][2]
    iq = D.recipe_iq("chain", a)
    rx, (ch0,) = _open(ctx, a, D.MAX_CAND, [rf0])
    slots = _Slots(ctx, rx)
    slots.run(iq)
    first = _check(ctx, ch0, code_a, UPSTREAM, t=slots.t)["rec"]
    assert D.best_set(first).max() >= 0
    # a second code between two boundaries takes effect at the next one: the same IQ, now no codeword of the loaded code
    ctx.set_ldpc_code(C.make_code(b)["nm"])
    slots.run(iq)
    second = _check(ctx, ch0, code_b, UPSTREAM, t=slots.t)["rec"]
    assert second.tobytes() != first.tobytes() and (D.best_set(second) < 0).all()
    ctx.set_ldpc_code(C.make_code(a)["nm"])
    # max_cand changed with the feature on: every buffer is made anew, the list is cut at 7
    _sync(ctx, 7)
    assert ctx.fetch_ft4_decode(ch0) is not None                       # (nothing is freed before the next boundary)
    slots.run(iq)
    r = _check(ctx, ch0, code_a, UPSTREAM, t=slots.t, max_cand=7)
    assert len(r["cands"]) == 7 and len(r["rec"]) >= 7
    _sync(ctx, D.MAX_CAND)
    # a channel closed and another opened between slots: the new one has records of its own from its first whole frame on
    ctx.channel_close(ch0)
    ch1 = ctx.channel_open(rx, rf1, "FT4")
    assert ctx.fetch_ft4_decode(ch1) is None
    slots.run(iq)
    slots.run(iq)
    r1 = _check(ctx, ch1, code_a, UPSTREAM, t=slots.t)
    for audio, t0, amp, mseed in D.RECIPES["chain"][2][1][1]:
        assert D.find_message(r1["rec"], D.message(mseed)), audio


def test_errors(xctx):
    from cwsl_digi_amd.api import CwslGpuError
    ctx = xctx

    def raises(status, fn, *a):
        with pytest.raises(CwslGpuError) as e:
            fn(*a)
        assert e.value.status == status

    raises(ARG, ctx.enable_ft4_decode, True, *UPSTREAM)                # no code, no sync stage, no soft bits
    ctx.enable_ft4_decode(False)                                       # switching it off is always allowed
    ctx.set_ldpc_code(C.make_code(C.SEEDS[0])["nm"])
    raises(ARG, ctx.enable_ft4_decode, True, *UPSTREAM)                # a code, but no sync stage
    _sync(ctx, 4)
    raises(ARG, ctx.enable_ft4_decode, True, *UPSTREAM)                # ... and no FT4 soft bits
    ctx.enable_ft8_softbits(True)
    raises(ARG, ctx.enable_ft4_decode, True, *UPSTREAM)                # FT8 soft bits are not FT4 soft bits
    ctx.enable_ft4_softbits(True)
    for bad in ((0, 8, 20), (201, 8, 20), (30, -1, 20), (30, 18, 20), (30, 8, -1), (30, 8, 34)):
        raises(ARG, ctx.enable_ft4_decode, True, *bad)
    # state unchanged by every refusal: a boundary still makes no decode records
    rx = ctx.receiver_open(FS, BLK, 0)
    c4, c8 = ctx.channel_open(rx, D.RECIPES["small"][2][0][0], "FT4"), ctx.channel_open(rx, -3000, "FT8")
    ctx.slot_boundary("FT4", 10)
    slots = _Slots(ctx, rx)
    assert slots.run(D.recipe_iq("small", C.SEEDS[0])) == 1
    assert ctx.fetch_ft4_decode(c4) is None and ctx.fetch_ft4_softbits(c4) is not None
    ctx.enable_ft4_decode(True, 200, 17, 33)
    ctx.enable_ft4_decode(True, 1, 0, 0)
    raises(MODE, ctx.fetch_ft4_decode, c8)                             # a fetch on an FT8 channel
    assert ctx.fetch_ft4_decode(c4) is None                            # enabled, but no boundary since
    # a context without a code keeps refusing after the sync stage and soft bits are on
    import cwsl_digi_amd as P
    other = P.Context(0)
    try:
        _sync(other, 4)
        other.enable_ft4_softbits(True)
        raises(ARG, other.enable_ft4_decode, True, *UPSTREAM)
    finally:
        other.close()
