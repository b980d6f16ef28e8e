"""GPU: FT8 OSD (cwslg_osd_msg) through the C ABI against the numpy restatement (tests/osd_ref.py), on (174, 91) codes made from a seed
(tests/ldpc_cases.py).  PARITY UNPINNED by the reference; against the restatement every record is BYTE-EQUAL -- no tolerance anywhere: the
stand-alone batches on the shared metric sets (tests/osd_cases.py), and the chain's records against the restatement applied to the GPU's own
soft-bit and decode records."""
import numpy as np
import pytest

import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O

pytestmark = pytest.mark.gpu
FS, BLK = OC.CHAIN_FS, OC.CHAIN_BLK
U32 = np.uint32
ARG, MODE = -6, -5


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


def _same(got, want):
    assert got.dtype == want.dtype == O.OSD_DTYPE and got.shape == want.shape, (got.shape, want.shape)
    bad = [q for q in range(len(want)) if got[q].tobytes() != want[q].tobytes()]
    assert not bad, (bad[:5], [(got[q], want[q]) for q in bad[:3]])


# ---- flat batches -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", C.SEEDS)
@pytest.mark.parametrize("order", OC.ORDERS)
@pytest.mark.parametrize("n", OC.BATCHES)
def test_batch_osd_is_the_restatement(xctx, n, order, seed):
    """cwslg_osd_decode on the first n of the vetted sets: empty, one wave, a partial and a full workgroup, the step into the next, three."""
    xctx.set_ldpc_code(C.make_code(seed)["nm"])
    got = xctx.osd_decode(OC.metric_sets(seed)[0][:n], order)
    _same(got, OC.reference_records(seed, order)[:n])


@pytest.mark.parametrize("seed", C.SEEDS)
def test_every_set_and_the_not_attempted_ones(xctx, seed):
    """All twelve sets at every order: the NaN, inf and -inf sets come back not attempted, between attempted neighbours."""
    xctx.set_ldpc_code(C.make_code(seed)["nm"])
    llr = OC.metric_sets(seed)[0]
    for order in OC.ORDERS:
        got = xctx.osd_decode(llr, order)
        _same(got, OC.reference_records(seed, order))
        for name in ("nan", "inf", "ninf"):
            assert got[OC.IDX[name]].tobytes() == O.NOT_ATTEMPTED.tobytes()
    # the last three alone, reversed: a workgroup whose waves all leave early
    _same(xctx.osd_decode(llr[:8:-1], 2), OC.reference_records(seed, 2)[:8:-1])


def test_reloading_a_code_replaces_the_generator(xctx):
    a, b = C.SEEDS
    llr = OC.metric_sets(a)[0]
    xctx.set_ldpc_code(C.make_code(a)["nm"])
    first = xctx.osd_decode(llr, 2)
    _same(first, OC.reference_records(a, 2))
    xctx.set_ldpc_code(C.make_code(b)["nm"])
    second = xctx.osd_decode(llr, 2)
    _same(second, O.decode(OC.generator(b), llr, 2))
    assert first.tobytes() != second.tobytes()
    xctx.set_ldpc_code(C.make_code(a)["nm"])
    _same(xctx.osd_decode(llr, 2), OC.reference_records(a, 2))


# ---- through the chain --------------------------------------------------------------------------------------------------------------------------
def _chain(ctx, seed, max_cand, order=OC.CHAIN_ORDER, osd_min_nsync=OC.CHAIN_OSD_MIN_NSYNC, osd=True, syncmin=OC.CHAIN_SYNC["syncmin"], quiet=False):
    ctx.enable_sync(True, syncmin, max_cand, OC.CHAIN_SYNC["f_lo"], OC.CHAIN_SYNC["f_hi"])
    ctx.enable_ft8_softbits(True)
    ctx.set_ldpc_code(C.make_code(seed)["nm"])
    ctx.enable_ft8_decode(True, OC.CHAIN_MAX_ITER, OC.CHAIN_MIN_NSYNC)
    if osd:
        ctx.enable_ft8_osd(True, order, osd_min_nsync)
    rx = ctx.receiver_open(FS, BLK, 0)
    chans = [ctx.channel_open(rx, rf, "FT8") for rf, _ in OC.CHAIN]
    if quiet:
        chans.append(ctx.channel_open(rx, OC.QUIET_RF, "FT8"))
    ctx.slot_boundary("FT8", 1)
    _push(ctx, rx, OC.chain_iq(seed))
    ctx.slot_boundary("FT8", 16)
    return rx, chans


def _check_channel(ctx, ch, seed, max_cand, order, osd_min_nsync, epoch=1):
    """OSD, decode and soft-bit records, list and frame of one epoch; every OSD record is the restatement on the GPU's own soft-bit and decode
    records -- the not-attempted ones included."""
    fr = ctx.fetch_frame(ch)
    cands, t_c = ctx.fetch_candidates(ch, max_cand, with_epoch=True)
    llr, sigma, nsync, t_s = ctx.fetch_ft8_softbits(ch, max_cand, with_epoch=True)
    msg, t_m = ctx.fetch_ft8_decode(ch, max_cand, with_epoch=True)
    got = ctx.fetch_ft8_osd(ch, max_cand, with_epoch=True)
    assert got is not None, "no OSD records of the current epoch"
    rec, t_o = got
    assert t_o == t_m == t_s == t_c == fr["t_start"] == epoch
    assert len(rec) == len(msg) == len(cands) == len(llr)
    _same(rec, O.chain_records(OC.generator(seed), llr, order, nsync, msg, osd_min_nsync))
    return cands, rec, msg, nsync


@pytest.mark.parametrize("seed", C.SEEDS)
def test_chain_records_are_the_restatement_and_the_messages_come_out(xctx, seed):
    """Three FT8 channels whose weakened transmissions (vetted on the CPU in tests/test_osd_cases_inputs.py) fail belief propagation at 30
    iterations: their strongest candidates come out of OSD with crc_ok and the sent message; the strong ones are decoded by belief propagation and
    OSD does not attempt them; every record of every list equals the restatement."""
    _, chans = _chain(xctx, seed, 200)
    hows = set()
    for ch, (rf, txs) in zip(chans, OC.CHAIN):
        cands, rec, msg, nsync = _check_channel(xctx, ch, seed, 200, OC.CHAIN_ORDER, OC.CHAIN_OSD_MIN_NSYNC)
        assert len(cands) > 5 and (rec["how"] == 0xff).any() and (rec["how"] != 0xff).any()
        for audio, t0, amp, mseed in txs:
            q = [k for k, c in enumerate(cands) if c[0] == int(round(audio / 3.125))][0]
            if mseed in OC.CHAIN_RECOVERED[seed]:
                assert msg[q]["iters"] >= 1 and msg[q]["crc_ok"] == 0
                assert rec[q]["crc_ok"] == 1 and np.array_equal(R.unpack_bits(rec[q]["bits"]), C.chain_message(mseed)), rec[q]
                hows.add(int(rec[q]["how"]))
            if mseed in OC.CHAIN_BP:
                assert msg[q]["crc_ok"] == 1 and rec[q].tobytes() == O.NOT_ATTEMPTED.tobytes()          # decoded by BP: not attempted
    assert len(hows) >= 2
    # a caller's own smaller `max` cuts the records like the list
    two = xctx.fetch_ft8_osd(chans[0], 2)
    assert len(two) == 2 and two.tobytes() == xctx.fetch_ft8_osd(chans[0], 200)[:2].tobytes()


@pytest.mark.parametrize("order", [0, 1])
def test_chain_at_the_lower_orders(xctx, order):
    seed = C.SEEDS[0]
    _, chans = _chain(xctx, seed, 200, order=order)
    for ch in chans:
        cands, rec, msg, nsync = _check_channel(xctx, ch, seed, 200, order, OC.CHAIN_OSD_MIN_NSYNC)
        att = rec[rec["how"] != 0xff]
        assert len(att) and (att["how"] <= order).all()


# ---- gates and list edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_nsync", [0, 16, 22])
def test_min_nsync_everything_bp_left_then_nothing(xctx, min_nsync):
    """min_nsync 0: every candidate the decode attempted without crc_ok (the decode's own gate stays at 7); 16: some of them; 22: none."""
    seed = C.SEEDS[1]
    _, chans = _chain(xctx, seed, 200, osd_min_nsync=min_nsync)
    for ch in chans:
        cands, rec, msg, nsync = _check_channel(xctx, ch, seed, 200, OC.CHAIN_ORDER, min_nsync)
        if min_nsync == 0:
            assert ((rec["how"] != 0xff) == ((msg["iters"] >= 0) & (msg["crc_ok"] == 0))).all() and (rec["how"] != 0xff).any()
        elif min_nsync == 16:
            assert ((rec["how"] != 0xff) == ((msg["iters"] >= 0) & (msg["crc_ok"] == 0) & (nsync >= 16))).all()
        else:
            assert (nsync < 22).all() and rec.tobytes() == np.repeat(O.NOT_ATTEMPTED, len(rec)).tobytes()


@pytest.mark.parametrize("max_cand", [1, 5])
def test_cut_lists(xctx, max_cand):
    seed = C.SEEDS[0]
    _, chans = _chain(xctx, seed, max_cand)
    for ch in chans:
        cands, rec, msg, nsync = _check_channel(xctx, ch, seed, max_cand, OC.CHAIN_ORDER, OC.CHAIN_OSD_MIN_NSYNC)
        assert len(rec) == max_cand
        assert len(xctx.fetch_ft8_osd(ch, 600)) == max_cand                  # a larger `max` than the list


def test_a_channel_without_candidates(xctx):
    """At QUIET_SYNCMIN the noise-only channel's list is empty: no records, not an error, while its neighbours' records are the restatement."""
    seed = C.SEEDS[0]
    _, chans = _chain(xctx, seed, 200, syncmin=OC.QUIET_SYNCMIN, quiet=True)
    quiet = chans[-1]
    assert len(xctx.fetch_candidates(quiet, 200)) == 0
    rec, t_o = xctx.fetch_ft8_osd(quiet, 200, with_epoch=True)
    assert len(rec) == 0 and t_o == 1
    n = 0
    for ch in chans[:-1]:
        n += len(_check_channel(xctx, ch, seed, 200, OC.CHAIN_ORDER, OC.CHAIN_OSD_MIN_NSYNC)[0])
    assert n > 0


# ---- off means off ------------------------------------------------------------------------------------------------------------------------------
def test_off_means_off(xctx):
    """Consecutive slots of the chain case's IQ: OSD never enabled (two launches per boundary: soft bits + search count as one, the decode as one),
    enabled (three; records), disabled (two; nothing to fetch -- not the previous slot's records), enabled again.  Frames, lists, soft-bit and
    decode records do not depend on the feature.  Disabling the decode or the soft bits silences OSD although it stays enabled."""
    ctx = xctx
    seed = C.SEEDS[0]
    iq = OC.chain_iq(seed)
    rx, chans = _chain(ctx, seed, 200, osd=False)
    ch = chans[0]
    epoch = [16]

    def slot():
        before = ctx.stats()["sync_launches"]
        _push(ctx, rx, iq)
        epoch[0] += 15
        ctx.slot_boundary("FT8", epoch[0])
        ctx.synchronize()
        return ctx.stats()["sync_launches"] - before

    def state():
        cands = ctx.fetch_candidates(ch, 200)
        llr, sigma, nsync = ctx.fetch_ft8_softbits(ch, 200)
        msg = ctx.fetch_ft8_decode(ch, 200)
        return ([tuple(np.float32(x).view(U32) if isinstance(x, float) else x for x in c) for c in cands], llr.tobytes(), sigma.tobytes(), nsync.tobytes(),
                msg.tobytes(), ctx.fetch_frame(ch)["i16"].tobytes())

    assert slot() == 2 and ctx.fetch_ft8_osd(ch) is None
    plain = state()
    ctx.enable_ft8_osd(True, 2, 7)
    assert ctx.fetch_ft8_osd(ch) is None                               # enabling computes nothing by itself: from the next boundary on
    assert slot() == 3
    assert state() == plain
    cands, rec, msg, nsync = _check_channel(ctx, ch, seed, 200, 2, 7, epoch=epoch[0] - 15)
    ctx.enable_ft8_osd(False)
    assert slot() == 2
    assert ctx.fetch_ft8_osd(ch) is None and state() == plain
    ctx.enable_ft8_osd(True, 2, 7)
    assert ctx.fetch_ft8_osd(ch) is None
    assert slot() == 3
    rec2, t_o = ctx.fetch_ft8_osd(ch, 200, with_epoch=True)
    assert t_o == epoch[0] - 15 and rec2.tobytes() == rec.tobytes() and state() == plain
    # the decode off at a boundary: no OSD records either, although OSD is still enabled
    ctx.enable_ft8_decode(False)
    assert slot() == 1
    assert ctx.fetch_ft8_osd(ch) is None and ctx.fetch_ft8_decode(ch) is None
    ctx.enable_ft8_decode(True, OC.CHAIN_MAX_ITER, OC.CHAIN_MIN_NSYNC)
    assert slot() == 3
    assert ctx.fetch_ft8_osd(ch, 200).tobytes() == rec.tobytes()
    # soft bits off: neither
    ctx.enable_ft8_softbits(False)
    assert slot() == 1
    assert ctx.fetch_ft8_osd(ch) is None and ctx.fetch_ft8_softbits(ch) is None


# ---- life cycle ---------------------------------------------------------------------------------------------------------------------------------
def test_life_cycle(xctx):
    """A new max_cand between two slots (the channel blocks are reallocated), a channel closed and another opened, a second code loaded between
    two boundaries: after each the records are the restatement on the GPU's own records of that slot."""
    ctx = xctx
    a, b = C.SEEDS
    rx, chans = _chain(ctx, a, 200)
    epoch = [16]

    def slot(seed):
        _push(ctx, rx, OC.chain_iq(seed))
        epoch[0] += 15
        ctx.slot_boundary("FT8", epoch[0])
        return epoch[0] - 15

    first = ctx.fetch_ft8_osd(chans[0], 200)
    ctx.enable_sync(True, OC.CHAIN_SYNC["syncmin"], 7, OC.CHAIN_SYNC["f_lo"], OC.CHAIN_SYNC["f_hi"])
    t = slot(a)
    for ch in chans:
        cands, rec, msg, nsync = _check_channel(ctx, ch, a, 7, OC.CHAIN_ORDER, OC.CHAIN_OSD_MIN_NSYNC, epoch=t)
        assert len(rec) == 7
    assert ctx.fetch_ft8_osd(chans[0], 7).tobytes() == first[:7].tobytes()
    # a channel closed, another opened at a dial offset that carries transmissions
    ctx.channel_close(chans[1])
    fresh = ctx.channel_open(rx, OC.CHAIN[1][0], "FT8")
    assert ctx.fetch_ft8_osd(fresh) is None
    t = slot(a)                                                         # (the new channel's first boundary discards its partial slot)
    t = slot(a)
    for ch in (chans[0], fresh, chans[2]):
        _check_channel(ctx, ch, a, 7, OC.CHAIN_ORDER, OC.CHAIN_OSD_MIN_NSYNC, epoch=t)
    # a second code between two boundaries: the next slot's records are the restatement under THAT code
    ctx.set_ldpc_code(C.make_code(b)["nm"])
    t = slot(b)
    for ch in (chans[0], fresh, chans[2]):
        cands, rec, msg, nsync = _check_channel(ctx, ch, b, 7, OC.CHAIN_ORDER, OC.CHAIN_OSD_MIN_NSYNC, epoch=t)
    assert (ctx.fetch_ft8_osd(chans[0], 7)["crc_ok"] == 1).any()


# ---- error paths --------------------------------------------------------------------------------------------------------------------------------
def test_errors(xctx):
    from cwsl_digi_amd.api import CwslGpuError
    ctx = xctx

    def raises(status, fn, *a):
        with pytest.raises(CwslGpuError) as e:
            fn(*a)
        assert e.value.status == status

    llr = OC.metric_sets(C.SEEDS[0])[0]
    raises(ARG, ctx.osd_decode, llr, 2)                                # no code loaded
    raises(ARG, ctx.enable_ft8_osd, True, 2, 7)
    ctx.enable_ft8_osd(False)                                          # switching it off is always allowed
    ctx.set_ldpc_code(C.make_code(C.SEEDS[0])["nm"])
    for order, ns in ((3, 7), (-1, 7), (2, 23), (2, -1)):
        raises(ARG, ctx.enable_ft8_osd, True, order, ns)
    raises(ARG, ctx.osd_decode, llr, 3)
    raises(ARG, ctx.osd_decode, llr, -1)
    assert len(ctx.osd_decode(llr[:0], 2)) == 0                         # n = 0 is legal
    ctx.enable_ft8_osd(True, 0, 0)                                      # a code of rank 83 and arguments in range: accepted without the sync stage
    ctx.enable_ft8_osd(True, 2, 22)
    # a rejected table leaves code and generator in force
    want = OC.reference_records(C.SEEDS[0], 2)
    for kind in C.BAD_TABLES:
        raises(ARG, ctx.set_ldpc_code, C.bad_table(C.SEEDS[1], kind))
        _same(ctx.osd_decode(llr, 2), want)
    # a fetch on an FT4 channel; a fetch before any boundary; a fetch whose epoch is not the one expected
    rx = ctx.receiver_open(FS, BLK, 0)
    c4, c8 = ctx.channel_open(rx, 3000, "FT4"), ctx.channel_open(rx, OC.CHAIN[0][0], "FT8")
    raises(MODE, ctx.fetch_ft8_osd, c4)
    assert ctx.fetch_ft8_osd(c8) is None
    ctx.enable_sync(True, OC.CHAIN_SYNC["syncmin"], 200, OC.CHAIN_SYNC["f_lo"], OC.CHAIN_SYNC["f_hi"])
    ctx.enable_ft8_softbits(True)
    ctx.enable_ft8_decode(True, 30, 7)
    ctx.enable_ft8_osd(True, 2, 7)
    ctx.slot_boundary("FT8", 1)
    assert ctx.fetch_ft8_osd(c8) is None                               # a boundary without a frame
    _push(ctx, rx, OC.chain_iq(C.SEEDS[0]))
    ctx.slot_boundary("FT8", 16)
    rec, t_o = ctx.fetch_ft8_osd(c8, 200, with_epoch=True)
    assert t_o == 1 and t_o != 16 and len(rec) > 0                      # the records carry the frame's START epoch: a consumer expecting 16 sees the mismatch
    ctx.enable_ft8_osd(False)
    _push(ctx, rx, OC.chain_iq(C.SEEDS[0]))
    ctx.slot_boundary("FT8", 31)
    assert ctx.fetch_ft8_osd(c8) is None and ctx.fetch_ft8_decode(c8, 200, with_epoch=True)[1] == 16   # never the older slot's records under the newer epoch
