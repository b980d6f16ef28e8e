"""GPU: FT4 OSD (cwslg_ft4_osd) through the C ABI at 48 kHz.  PARITY UNPINNED by the reference; every comparison is BYTE EQUALITY of whole 72-byte
records against tests/ft4_osd_cases.py:expected() -- the numpy restatement of cwslg_osd_msg (tests/osd_ref.py) per metric set under the
record-level gate -- applied to the GPU's own fetched cwslg_ft4_soft and cwslg_ft4_msg records (which are themselves compared with the decode's
restatement).  No tolerance anywhere.  The inputs are vetted on the CPU in tests/test_ft4_osd_inputs.py.  As for the decode, no frame reaches
sigma[s] == 0 through the chain (it takes 206 equal metrics): such a set is not attempted by the decode, hence not by OSD, and that rule is
exercised on hand-made records in the inputs test only.  Tests that look at gates, buffers and epochs rather than at the search run at order
1, which keeps the restatement on the host quick; the orders are compared on the main frame."""
import numpy as np
import pytest

import ft4_decode_cases as D
import ft4_osd_cases as X
import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O

pytestmark = pytest.mark.gpu
FS, BLK, N4 = X.FS, X.BLK, X.N4
U32 = np.uint32
ARG, MODE = -6, -5
DECODE = (X.MAX_ITER, X.MIN_NSYNC, X.MIN_NQUAL)
UPSTREAM = (X.ORDER, X.MIN_NSYNC, X.MIN_NQUAL)
NA = O.NOT_ATTEMPTED[0]


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


def _sync(ctx, max_cand, syncmin4=X.SYNCMIN_FT4):
    ctx.enable_sync(True, X.SYNC["syncmin"], max_cand, X.SYNC["f_lo"], X.SYNC["f_hi"])
    ctx.set_ft4_syncmin(syncmin4)                                      # (cwslg_enable_sync starts from the default threshold)


def _open(ctx, seed, max_cand, rfs, syncmin4=X.SYNCMIN_FT4, decode=DECODE, osd=UPSTREAM):
    """Sync stage, FT4 soft bits, the seed's code, the decode and (osd not None) OSD; one receiver, FT4 channels at rfs, the first frame begun."""
    _sync(ctx, max_cand, syncmin4)
    ctx.enable_ft4_softbits(True)
    ctx.set_ldpc_code(C.make_code(seed)["nm"])
    ctx.enable_ft4_decode(True, *decode)
    if osd:
        ctx.enable_ft4_osd(True, *osd)
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


def _same(got, want, dtype=X.OSD4_DTYPE):
    assert got.dtype == want.dtype == dtype and got.shape == want.shape, (got.shape, want.shape)
    bad = [q for q in range(len(want)) if got[q].tobytes() != want[q].tobytes()]
    assert not bad, (bad[:5], [(got[q], want[q]) for q in bad[:3]])


def _check(ctx, ch, seed, osd, decode=DECODE, t=None, max_cand=X.MAX_CAND):
    """OSD, decode, soft and sync records, list and frame of one epoch; every decode record is its restatement on the GPU's own soft record and
    every OSD record is expected() of the GPU's own soft and decode records -- the not-attempted ones included."""
    fr = ctx.fetch_frame(ch)
    cands, t_c = ctx.fetch_candidates(ch, max_cand, with_epoch=True)
    recs = ctx.fetch_ft4_sync(ch)
    llr, sigma, nsync, nqual, t_s = ctx.fetch_ft4_softbits(ch, with_epoch=True)
    msg, t_m = ctx.fetch_ft4_decode(ch, with_epoch=True)
    got = ctx.fetch_ft4_osd(ch, with_epoch=True)
    assert got is not None, "no OSD records of the current epoch"
    rec, t_o = got
    assert t_o == t_m == t_s == t_c == fr["t_start"] and (t is None or t_o == t), (t_o, t_m, t_s, t_c, fr["t_start"], t)
    assert len(rec) == len(msg) == len(recs) == len(llr)
    soft = D.soft_dict(llr, sigma, nsync, nqual)
    _same(msg, D.expected(soft, C.make_code(seed)["code"], *decode), D.MSG4_DTYPE)
    _same(rec, X.expected(soft, msg, X.generator(seed), *osd))
    return dict(rec=rec, msg=msg, soft=soft, recs=recs, cands=cands, fr=fr)


def _na(rec):
    """Which sets are the not-attempted pattern, checked field by field: bool[n, 3]."""
    s = rec["set"]
    na = s["how"] == 0xff
    assert (na == (s["nharderr"] == -1)).all() and (na == (s["nskip"] == -1)).all() and (s["flip"][na] == 0xff).all()
    assert not s["bits"][na].any() and not s["crc_ok"][na].any() and (s["dmin"][na].view(U32) == 0).all()
    return na


@pytest.mark.parametrize("seed", C.SEEDS)
def test_chain_ft4_osd_beside_ft8_osd(xctx, seed):
    """The two FT4 channels of the main frame beside an FT8 channel with FT8 decode and FT8 OSD on, in one context: both pointer tables and both
    chain modes of the kernel in the same pair of boundaries, each checked against its restatement.  The transmission BP fails in all three sets
    comes out under ft4_best_word flagged by OSD with the 91 bits sent; the one BP decodes comes out by BP with its OSD record not attempted;
    the record BP decodes in some sets only is not attempted in any set."""
    from cwsl_digi_amd.api import CwslGpuError, ft4_best_word
    ctx = xctx
    head = np.array(OC.chain_iq(seed)[:OC.CHAIN_N - N4])               # the FT8 slot: the FT8 OSD chain case's first half, then the FT4 frame
    tail = X.recipe_iq("main", seed)
    _sync(ctx, X.MAX_CAND)
    ctx.enable_ft4_softbits(True)
    ctx.enable_ft8_softbits(True)
    ctx.set_ldpc_code(C.make_code(seed)["nm"])
    ctx.enable_ft4_decode(True, *DECODE)
    ctx.enable_ft8_decode(True, 30, 7)
    ctx.enable_ft8_osd(True, 1, 7)
    ctx.enable_ft4_osd(True, *UPSTREAM)
    rx = ctx.receiver_open(FS, BLK, 0)
    c4 = [ctx.channel_open(rx, rf, "FT4") for rf in (X.RF_TX, X.RF_NOISE)]
    c8 = ctx.channel_open(rx, OC.CHAIN[0][0], "FT8")
    ctx.slot_boundary("FT8", 1)
    _push(ctx, rx, head)
    ctx.slot_boundary("FT4", 10)
    _push(ctx, rx, tail)
    ctx.slot_boundary("FT4", 17)
    ctx.slot_boundary("FT8", 16)
    r = _check(ctx, c4[0], seed, UPSTREAM, t=10)
    rec, msg = r["rec"], r["msg"]
    na = _na(rec)
    assert na.any() and not na.all() and (na.all(axis=1) | ~na.any(axis=1)).all()
    best, by = ft4_best_word(msg, rec)
    xb, xby = X.best_word(msg, rec)
    assert np.array_equal(best, xb) and np.array_equal(by, xby)
    sent = {m: (audio, D.message(m)) for audio, _, _, m in X.transmissions("main", seed)}
    for mseed in X.RECOVERED["main"][seed]:
        hits = X.find_word(msg, rec, sent[mseed][1])
        assert hits and hits[0][1] and abs(r["recs"][hits[0][0]]["f1_hz"] - sent[mseed][0]) <= 3.0, mseed
        q = hits[0][0]
        assert not msg["set"]["crc_ok"][q].any() and by[q] and rec["set"]["how"][q, best[q]] == X.HOW["main"][seed]
        assert ft4_best_word(msg[q], rec[q]) == (int(best[q]), True)
    for mseed in X.BP["main"][seed]:
        hits = X.find_word(msg, rec, sent[mseed][1])
        assert hits and not hits[0][1], mseed
        assert na[hits[0][0]].all() and all(rec["set"][hits[0][0], s] == NA for s in range(3))
    bp_ok = msg["set"]["crc_ok"] != 0
    some = bp_ok.any(axis=1) & ~bp_ok.all(axis=1)
    assert some.any() and na[some].all()                                # the record gate: a per-set gate would have attempted the failed sets
    assert X.per_set_gate(r["soft"], msg, X.MIN_NSYNC, X.MIN_NQUAL)[some].any()
    _check(ctx, c4[1], seed, UPSTREAM, t=10)                           # the noise channel: its own list, its own arrays
    # a caller's own smaller `max` cuts the records like the sync records
    two = ctx.fetch_ft4_osd(c4[0], 2)
    assert len(two) == 2 and two.tobytes() == rec[:2].tobytes()
    # the FT8 form beside it, in the same context
    cands, t_c = ctx.fetch_candidates(c8, 200, with_epoch=True)
    llr, sigma, nsync, t_s = ctx.fetch_ft8_softbits(c8, 200, with_epoch=True)
    msg8, t_m = ctx.fetch_ft8_decode(c8, 200, with_epoch=True)
    rec8, t_o = ctx.fetch_ft8_osd(c8, 200, with_epoch=True)
    assert t_o == t_m == t_s == t_c == 1 and len(rec8) == len(cands) > 0
    assert msg8.tobytes() == R.hard_records(C.make_code(seed)["code"], llr, 30, nsync, sigma, 7).tobytes()
    assert rec8.tobytes() == O.chain_records(X.generator(seed), llr, 1, nsync, msg8, 7).tobytes() and (rec8["how"] != 0xff).any()
    for fn, ch in ((ctx.fetch_ft4_osd, c8), (ctx.fetch_ft8_osd, c4[0])):
        with pytest.raises(CwslGpuError) as e:
            fn(ch)
        assert e.value.status == MODE


@pytest.mark.parametrize("order", [0, 1])
def test_lower_orders(xctx, order):
    seed = C.SEEDS[0]
    rx, (ch,) = _open(xctx, seed, X.MAX_CAND, [X.RF_TX], osd=(order, X.MIN_NSYNC, X.MIN_NQUAL))
    _Slots(xctx, rx).run(X.recipe_iq("main", seed))
    rec = _check(xctx, ch, seed, (order, X.MIN_NSYNC, X.MIN_NQUAL), t=10)["rec"]
    na = _na(rec)
    assert not na.all() and rec["set"]["how"][~na].max() == order
    assert (rec["set"]["flip"][~na][:, 1] == 0xff).all()                # no second flip below order 2


@pytest.mark.parametrize("seed", C.SEEDS)
def test_the_weak_frame_gives_the_other_flip_count(xctx, seed):
    """The second frame per code: the word comes back with the flip count the main frame does not show (how is 1 once and 2 once per code)."""
    rx, (ch,) = _open(xctx, seed, X.MAX_CAND, [X.RF_TX])
    _Slots(xctx, rx).run(X.recipe_iq("weak", seed))
    r = _check(xctx, ch, seed, UPSTREAM, t=10)
    (mseed,) = X.RECOVERED["weak"][seed]
    hits = X.find_word(r["msg"], r["rec"], D.message(mseed))
    assert hits and hits[0][1]
    q = hits[0][0]
    s = int(X.best_word(r["msg"], r["rec"])[0][q])
    assert r["rec"]["set"]["how"][q, s] == X.HOW["weak"][seed] != X.HOW["main"][seed]


@pytest.mark.parametrize("max_cand", [1, 2, 5])
def test_smallest_shapes_cut_lists_and_holes(xctx, max_cand):
    """9, 18 and 45 waves per channel: the last workgroup is partly empty.  The lists are longer than max_cand and are cut; at 5 the candidates
    have one to three records, so the slot array has holes.  Gates (0, 0) in both stages: every record's three sets run the whole search."""
    seed = C.SEEDS[0]
    rx, chans = _open(xctx, seed, max_cand, [X.RF_TX, X.RF_NOISE], decode=(X.MAX_ITER, 0, 0), osd=(X.ORDER, 0, 0))
    _Slots(xctx, rx).run(X.recipe_iq("main", seed))
    counts = set()
    for ch in chans:
        r = _check(xctx, ch, seed, (X.ORDER, 0, 0), decode=(X.MAX_ITER, 0, 0), t=10, max_cand=max_cand)
        assert len(r["cands"]) == max_cand and len(r["rec"]) >= max_cand
        counts |= set(np.bincount([h["cand"] for h in r["recs"]], minlength=max_cand).tolist())
        na = _na(r["rec"])
        assert (na == (r["msg"]["set"]["crc_ok"] != 0).any(axis=1)[:, None]).all()     # all attempted, but for a record BP decoded
    assert counts <= {1, 2, 3} and (max_cand < 5 or len(counts) >= 2), counts


def test_candidates_with_zero_one_two_and_three_records(xctx):
    """The "carriers" frame at max_cand 17 (153 waves, the last workgroup partly empty, the list cut): a wholly empty candidate lies between
    occupied ones in the slot array -- its nine waves leave, and the fetch's walk skips it, keeping record q with entry q of the sync fetch.
    Once with every record attempted (order 1) and once with upstream's gates (order 2)."""
    seed = C.SEEDS[0]
    (rf, _), = D.RECIPES["carriers"][2]
    mc = X.HOLES_MAX_CAND
    rx, (ch,) = _open(xctx, seed, mc, [rf])
    slots = _Slots(xctx, rx)
    for decode, osd in (((X.MAX_ITER, 0, 0), (1, 0, 0)), (DECODE, UPSTREAM)):
        xctx.enable_ft4_decode(True, *decode)
        xctx.enable_ft4_osd(True, *osd)
        slots.run(X.recipe_iq("carriers", seed))
        r = _check(xctx, ch, seed, osd, decode=decode, t=slots.t, max_cand=mc)
        nrec = np.bincount([h["cand"] for h in r["recs"]], minlength=mc)
        assert len(r["cands"]) == mc and set(nrec.tolist()) == {0, 1, 2, 3}, nrec
        hole = int(np.nonzero(nrec == 0)[0][0])
        assert 0 < hole < mc - 1 and nrec[hole + 1:].sum() > 0 and len(r["rec"]) == nrec.sum()
        if osd == (1, 0, 0):
            assert not _na(r["rec"]).any()


def test_noise_only_channel_has_zero_records(xctx):
    seed = C.SEEDS[0]
    rx, (a, b) = _open(xctx, seed, 2, [X.RF_TX, X.RF_NOISE], syncmin4=X.SYNCMIN_QUIET)
    _Slots(xctx, rx).run(X.recipe_iq("small", seed))
    assert len(_check(xctx, a, seed, UPSTREAM, t=10, max_cand=2)["rec"]) >= 1
    assert xctx.fetch_candidates(b, 2) == [] and xctx.fetch_ft4_sync(b) == []
    rec, t_o = xctx.fetch_ft4_osd(b, with_epoch=True)                  # n == 0, no error
    assert rec.shape == (0,) and rec.dtype == X.OSD4_DTYPE and t_o == 10


def test_gates(xctx):
    """One channel, the main frame under four OSD gate settings (each applies from the next boundary on), the decode attempting every record.
    Order 1: the gates do not depend on the order."""
    ctx = xctx
    seed = C.SEEDS[0]
    decode = (X.MAX_ITER, 0, 0)
    rx, (ch,) = _open(ctx, seed, X.MAX_CAND, [X.RF_TX], decode=decode, osd=None)
    slots = _Slots(ctx, rx)
    iq = X.recipe_iq("main", seed)
    for gates in ((0, 0), (17, 0), (0, 33), (8, 20)):
        ctx.enable_ft4_osd(True, 1, *gates)
        slots.run(iq)
        r = _check(ctx, ch, seed, (1,) + gates, decode=decode, t=slots.t)
        na = _na(r["rec"])
        bp = (r["msg"]["set"]["crc_ok"] != 0).any(axis=1)
        assert len(r["rec"]) > 20 and bp.any() and (r["msg"]["set"]["iters"] >= 0).all()
        if gates == (0, 0):
            assert (na == bp[:, None]).all()                            # everything BP left, and nothing else
        elif gates in ((17, 0), (0, 33)):
            assert na.all()
        else:
            low = (r["soft"]["nsync"] < 8) | (r["soft"]["nqual"] < 20)
            assert low.any() and not low.all() and (na == (bp | low)[:, None]).all()


def test_off_means_off(xctx):
    """OSD never enabled: the launches a boundary had, nothing to fetch.  On: exactly one launch more.  Off again, the decode off, soft bits off,
    the coherent stage off: the earlier launch counts and CWSLG_ERR_NO_FRAME -- never the previous slot's records.  Frames, lists, sync, soft and
    decode records do not depend on it."""
    ctx = xctx
    seed = C.SEEDS[0]
    iq = X.recipe_iq("main", seed)
    rx, (ch,) = _open(ctx, seed, X.MAX_CAND, [X.RF_TX], osd=None)
    slots = _Slots(ctx, rx)
    osd = (1, X.MIN_NSYNC, X.MIN_NQUAL)

    def state():
        soft = ctx.fetch_ft4_softbits(ch)
        msg = ctx.fetch_ft4_decode(ch)
        cands = [tuple(np.float32(x).view(U32) if isinstance(x, float) else x for x in c) for c in ctx.fetch_candidates(ch, X.MAX_CAND)]
        return (ctx.fetch_frame(ch)["i16"].tobytes(), cands, ctx.fetch_ft4_sync(ch), None if soft is None else tuple(x.tobytes() for x in soft),
                None if msg is None else msg.tobytes())

    off = slots.run(iq)
    assert off == 2 and ctx.fetch_ft4_osd(ch) is None                  # the sync stage and the decode
    plain = state()
    assert plain[3] is not None and plain[4] is not None and len(plain[2]) > 20
    ctx.enable_ft4_osd(True, *osd)
    assert ctx.fetch_ft4_osd(ch) is None                               # enabling computes nothing by itself: from the next boundary on
    assert slots.run(iq) == off + 1
    assert state() == plain
    rec = _check(ctx, ch, seed, osd, t=slots.t)["rec"]
    ctx.enable_ft4_osd(False)
    assert slots.run(iq) == off
    assert ctx.fetch_ft4_osd(ch) is None and state() == plain          # not the previous slot's records under this epoch
    ctx.enable_ft4_osd(True, *osd)
    assert ctx.fetch_ft4_osd(ch) is None
    assert slots.run(iq) == off + 1
    assert _check(ctx, ch, seed, osd, t=slots.t)["rec"].tobytes() == rec.tobytes()
    ctx.enable_ft4_decode(False)                                       # the decode off at a boundary, OSD still enabled
    assert slots.run(iq) == off - 1
    assert ctx.fetch_ft4_osd(ch) is None and ctx.fetch_ft4_decode(ch) is None and state()[:4] == plain[:4]
    ctx.enable_ft4_decode(True, *DECODE)
    assert slots.run(iq) == off + 1
    assert _check(ctx, ch, seed, osd, t=slots.t)["rec"].tobytes() == rec.tobytes()
    ctx.enable_ft4_softbits(False)                                     # soft bits off at a boundary, decode and OSD still enabled
    assert slots.run(iq) == off - 1
    assert ctx.fetch_ft4_osd(ch) is None and ctx.fetch_ft4_softbits(ch) is None and state()[:3] == plain[:3]
    ctx.enable_ft4_softbits(True)
    assert slots.run(iq) == off + 1
    assert _check(ctx, ch, seed, osd, t=slots.t)["rec"].tobytes() == rec.tobytes()
    ctx.enable_ft4_coherent(False)                                     # coherent stage off: no records of any kind
    assert slots.run(iq) == off - 1
    assert ctx.fetch_ft4_osd(ch) is None and ctx.fetch_ft4_decode(ch) is None
    assert ctx.fetch_candidates(ch, X.MAX_CAND, with_epoch=True)[1] == slots.t


def test_life_cycle(xctx):
    """A second code between two boundaries (the generator is replaced), a new max_cand, a channel closed and another opened, and a table of
    rank 82 that switches OSD off while the decode goes on.  Order 1 keeps the restatement quick; the code and the buffers do not depend on it."""
    from cwsl_digi_amd.api import CwslGpuError
    ctx = xctx
    b, a = C.SEEDS                                                      # (under the second code the main frame's word needs one flip: order 1 finds it)
    assert X.HOW["main"][a] == 1
    osd = (1, X.MIN_NSYNC, X.MIN_NQUAL)
    iq = X.recipe_iq("main", a)
    rx, (ch0,) = _open(ctx, a, X.MAX_CAND, [X.RF_TX], osd=osd)
    slots = _Slots(ctx, rx)
    assert slots.run(iq) == 3
    first = _check(ctx, ch0, a, osd, t=slots.t)["rec"]
    assert (first["set"]["crc_ok"] != 0).any()
    # a second code between two boundaries takes effect at the next one: tables AND generator
    ctx.set_ldpc_code(C.make_code(b)["nm"])
    slots.run(iq)
    second = _check(ctx, ch0, b, osd, t=slots.t)["rec"]
    assert second.tobytes() != first.tobytes()
    ctx.set_ldpc_code(C.make_code(a)["nm"])
    # max_cand changed with the feature on: every buffer is made anew, the list is cut at 7
    _sync(ctx, 7)
    assert ctx.fetch_ft4_osd(ch0) is not None                          # (nothing is freed before the next boundary)
    slots.run(iq)
    r = _check(ctx, ch0, a, osd, t=slots.t, max_cand=7)
    assert len(r["cands"]) == 7 and len(r["rec"]) >= 7
    _sync(ctx, X.MAX_CAND)
    # a channel closed and another opened between slots: the new one has records of its own from its first whole frame on
    ctx.channel_close(ch0)
    ch1 = ctx.channel_open(rx, X.RF_TX, "FT4")
    assert ctx.fetch_ft4_osd(ch1) is None
    slots.run(iq)
    slots.run(iq)
    again = _check(ctx, ch1, a, osd, t=slots.t)["rec"]
    assert (again["set"]["crc_ok"] != 0).any() and (again["set"]["how"] == 0xff).any()
    # a table the decode takes and OSD cannot run on: OSD is switched off, the decode goes on under that table
    nm = X.rank_deficient_table()
    ctx.set_ldpc_code(nm)
    assert slots.run(iq) == 2
    assert ctx.fetch_ft4_osd(ch1) is None
    llr, sigma, nsync, nqual = ctx.fetch_ft4_softbits(ch1)
    _same(ctx.fetch_ft4_decode(ch1), D.expected(D.soft_dict(llr, sigma, nsync, nqual), R.Code(np.array(nm)), *DECODE), D.MSG4_DTYPE)
    with pytest.raises(CwslGpuError) as e:
        ctx.enable_ft4_osd(True, *osd)
    assert e.value.status == ARG
    ctx.set_ldpc_code(C.make_code(a)["nm"])                            # a code of rank 83 again: OSD stays off until it is enabled
    assert slots.run(iq) == 2 and ctx.fetch_ft4_osd(ch1) is None
    ctx.enable_ft4_osd(True, *osd)
    assert slots.run(iq) == 3
    assert (_check(ctx, ch1, a, osd, t=slots.t)["rec"]["set"]["crc_ok"] != 0).any()


def test_errors(xctx):
    from cwsl_digi_amd.api import CwslGpuError
    from cwsl_digi_amd import build as B
    import ctypes
    ctx = xctx

    def raises(status, fn, *a):
        with pytest.raises(CwslGpuError) as e:
            fn(*a)
        assert e.value.status == status

    raises(ARG, ctx.enable_ft4_osd, True, *UPSTREAM)                   # no code loaded
    ctx.enable_ft4_osd(False)                                          # switching it off is always allowed
    ctx.set_ldpc_code(C.make_code(C.SEEDS[0])["nm"])
    for bad in ((3, 8, 20), (-1, 8, 20), (2, -1, 20), (2, 18, 20), (2, 8, -1), (2, 8, 34)):
        raises(ARG, ctx.enable_ft4_osd, True, *bad)
    ctx.enable_ft4_osd(True, 0, 0, 0)                                  # a code of rank 83 and arguments in range: accepted without the sync stage
    ctx.enable_ft4_osd(True, 2, 17, 33)
    lib = ctypes.CDLL(B.LIB)
    assert lib.cwslg_enable_ft4_osd(None, 1, 2, 8, 20) == ARG and lib.cwslg_fetch_ft4_osd(None, 0, None, 0, None, None) == ARG
    # enabled, but without soft bits and decode a boundary makes no OSD records and no launch more
    _sync(ctx, 4)
    rx = ctx.receiver_open(FS, BLK, 0)
    c4, c8 = ctx.channel_open(rx, X.RF_TX, "FT4"), ctx.channel_open(rx, -3000, "FT8")
    raises(MODE, ctx.fetch_ft4_osd, c8)                                # a fetch on an FT8 channel
    assert ctx.fetch_ft4_osd(c4) is None                               # a fetch before any boundary
    ctx.slot_boundary("FT4", 10)
    slots = _Slots(ctx, rx)
    assert slots.run(X.recipe_iq("main", C.SEEDS[0])) == 1
    assert ctx.fetch_ft4_osd(c4) is None and ctx.fetch_ft4_sync(c4)
    ctx.enable_ft4_softbits(True)
    ctx.enable_ft4_decode(True, *DECODE)
    assert ctx.fetch_ft4_osd(c4) is None                               # all on, but no boundary since
    assert slots.run(X.recipe_iq("main", C.SEEDS[0])) == 3
    rec, t_o = ctx.fetch_ft4_osd(c4, with_epoch=True)
    assert t_o == slots.t and (rec["set"]["how"] == 0xff).all()        # gates 17 / 33: nothing is attempted
    # a context without a code keeps refusing
    import cwsl_digi_amd as P
    other = P.Context(0)
    try:
        _sync(other, 4)
        other.enable_ft4_softbits(True)
        raises(ARG, other.enable_ft4_osd, True, *UPSTREAM)
    finally:
        other.close()
