"""GPU: the FT8 decode (cwslg_ft8_msg) through the C ABI at 48 kHz against the numpy restatement (tests/ldpc_ref.py), on (174, 91) codes made
from a seed (tests/ldpc_cases.py; the upstream table is the integrator's data and is not in this repository).  PARITY UNPINNED by the reference;
against the restatement every record is BYTE-EQUAL -- no tolerance anywhere: the stand-alone batch on the shared metric sets, and the chain's
records against the restatement applied to the GPU's own soft-bit records."""
import numpy as np
import pytest

import ldpc_cases as C
import ldpc_ref as R

pytestmark = pytest.mark.gpu
FS, BLK, N8 = C.CHAIN_FS, C.CHAIN_BLK, C.CHAIN_N
U32 = np.uint32


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
    assert got.dtype == want.dtype == R.MSG_DTYPE and got.shape == want.shape, (got.shape, want.shape)
    bad = [q for q in range(len(want)) if got[q].tobytes() != want[q].tobytes()]
    assert not bad, (bad[:5], [(got[q], want[q]) for q in bad[:3]])


@pytest.mark.parametrize("max_iter", C.MAX_ITERS)
@pytest.mark.parametrize("n", C.BATCHES)
def test_batch_decode_is_the_restatement(xctx, n, max_iter):
    """cwslg_ldpc_decode on the first n of the vetted sets: empty, one wave, a partial and a full workgroup, the step into the next, three."""
    seed = C.SEEDS[0]
    xctx.set_ldpc_code(C.make_code(seed)["nm"])
    got = xctx.ldpc_decode(C.metric_sets(seed)[0][:n], max_iter)
    _same(got, C.reference_records(seed, max_iter)[:n])


def test_reloading_a_code_takes_effect(xctx):
    """The first code's metric sets under the second code: the records are the restatement's under THAT code and differ from the first's; back
    again, the first's."""
    a, b = C.SEEDS
    llr = C.metric_sets(a)[0]
    xctx.set_ldpc_code(C.make_code(a)["nm"])
    first = xctx.ldpc_decode(llr, 30)
    _same(first, C.reference_records(a, 30))
    xctx.set_ldpc_code(C.make_code(b)["nm"])
    second = xctx.ldpc_decode(llr, 30)
    _same(second, R.decode(C.make_code(b)["code"], llr, 30))
    assert first.tobytes() != second.tobytes()
    xctx.set_ldpc_code(C.make_code(a)["nm"])
    _same(xctx.ldpc_decode(llr, 30), C.reference_records(a, 30))


def _chain(ctx, seed, max_cand, max_iter=30, min_nsync=7, decode=True):
    ctx.enable_sync(True, C.CHAIN_SYNC["syncmin"], max_cand, C.CHAIN_SYNC["f_lo"], C.CHAIN_SYNC["f_hi"])
    ctx.enable_ft8_softbits(True)
    ctx.set_ldpc_code(C.make_code(seed)["nm"])
    if decode:
        ctx.enable_ft8_decode(True, max_iter, min_nsync)
    rx = ctx.receiver_open(FS, BLK, 0)
    chans = [ctx.channel_open(rx, rf, "FT8") for rf, _ in C.CHAIN]
    ctx.slot_boundary("FT8", 1)
    _push(ctx, rx, C.chain_iq(seed))
    ctx.slot_boundary("FT8", 16)
    return rx, chans


def _check_channel(ctx, ch, code, max_cand, max_iter, min_nsync):
    """Decode records, soft-bit records, list and frame of one epoch; every decode record is the restatement of the GPU's own soft-bit record."""
    fr = ctx.fetch_frame(ch)
    cands, t_c = ctx.fetch_candidates(ch, max_cand, with_epoch=True)
    llr, sigma, nsync, t_s = ctx.fetch_ft8_softbits(ch, max_cand, with_epoch=True)
    got = ctx.fetch_ft8_decode(ch, max_cand, with_epoch=True)
    assert got is not None, "no decode records of the current epoch"
    rec, t_m = got
    assert t_m == t_s == t_c == fr["t_start"] == 1
    assert len(rec) == len(cands) == len(llr)
    _same(rec, R.hard_records(code, llr, max_iter, nsync, sigma, min_nsync))
    return cands, rec, nsync


@pytest.mark.parametrize("max_cand", [5, 200])
def test_chain_records_are_the_restatement_and_the_messages_come_out(xctx, max_cand):
    """Three FT8 channels, two or three transmissions each that carry real codewords in noise at which the strongest candidate needs at least one
    iteration (vetted on the CPU in tests/test_ldpc_cases_inputs.py).  Every record of every list equals the restatement on the GPU's own
    soft-bit record with the nsync filter; per transmission the strongest candidate has crc_ok and the 91 bits sent."""
    seed = C.SEEDS[0]
    code = C.make_code(seed)["code"]
    _, chans = _chain(xctx, seed, max_cand)
    for ch, (rf, txs) in zip(chans, C.CHAIN):
        cands, rec, nsync = _check_channel(xctx, ch, code, max_cand, 30, 7)
        assert len(cands) == 5 if max_cand == 5 else len(cands) > 5
        if max_cand == 200:
            assert (rec["iters"] == -1).any() and ((rec["iters"] == -1) == (nsync < 7)).all()
        for audio, t0, amp, mseed in txs:
            q = [k for k, c in enumerate(cands) if c[0] == int(round(audio / 3.125))][0]
            assert rec[q]["crc_ok"] == 1 and rec[q]["nbad"] == 0 and rec[q]["iters"] >= 1, rec[q]
            assert np.array_equal(R.unpack_bits(rec[q]["bits"]), C.chain_message(mseed))
    # a caller's own smaller `max` cuts the records like the list
    two = xctx.fetch_ft8_decode(chans[0], 2)
    assert len(two) == 2 and two.tobytes() == xctx.fetch_ft8_decode(chans[0], max_cand)[:2].tobytes()


@pytest.mark.parametrize("min_nsync", [0, 22])
def test_min_nsync_everything_then_nothing(xctx, min_nsync):
    seed = C.SEEDS[1]
    code = C.make_code(seed)["code"]
    _, chans = _chain(xctx, seed, 200, max_iter=5, min_nsync=min_nsync)
    for ch in chans:
        cands, rec, nsync = _check_channel(xctx, ch, code, 200, 5, min_nsync)
        assert len(rec) > 5
        if min_nsync == 0:
            assert (rec["iters"] >= 0).all()                            # (no candidate of these lists has sigma == 0)
        else:
            assert (rec["iters"] == -1).all() and not rec["bits"].any() and not rec["crc_ok"].any()


def test_off_means_off(xctx):
    """Four consecutive slots of the chain case's IQ: decode never enabled (launches per boundary noted, nothing to fetch), enabled (one launch
    more; records), disabled (the first slot's launches; nothing to fetch -- not the previous slot's records), enabled again (nothing until the
    next boundary, then records).  Lists and soft-bit records do not depend on the feature."""
    ctx = xctx
    seed = C.SEEDS[0]
    code = C.make_code(seed)["code"]
    iq = C.chain_iq(seed)
    rx, chans = _chain(ctx, seed, 200, decode=False)
    ch = chans[1]
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
        return [tuple(np.float32(x).view(U32) if isinstance(x, float) else x for x in c) for c in cands], llr.tobytes(), sigma.tobytes(), nsync.tobytes()

    off = slot()
    assert off == 1 and ctx.fetch_ft8_decode(ch) is None
    plain = state()
    ctx.enable_ft8_decode(True, 30, 7)
    assert ctx.fetch_ft8_decode(ch) is None                            # enabling computes nothing by itself: from the next boundary on
    assert slot() == off + 1
    assert state() == plain                                            # the same IQ: the same list and soft-bit records, decode on or off
    rec, t_m = ctx.fetch_ft8_decode(ch, 200, with_epoch=True)
    assert t_m == epoch[0] - 15 == ctx.fetch_frame(ch)["t_start"]
    llr, sigma, nsync = ctx.fetch_ft8_softbits(ch, 200)
    _same(rec, R.hard_records(code, llr, 30, nsync, sigma, 7))
    ctx.enable_ft8_decode(False)
    assert slot() == off
    assert ctx.fetch_ft8_decode(ch) is None and state() == plain
    ctx.enable_ft8_decode(True, 30, 7)
    assert ctx.fetch_ft8_decode(ch) is None
    assert slot() == off + 1
    rec2, t_m = ctx.fetch_ft8_decode(ch, 200, with_epoch=True)
    assert t_m == epoch[0] - 15 and rec2.tobytes() == rec.tobytes()
    # soft bits off at a boundary: no decode records either, although decode is still enabled
    ctx.enable_ft8_softbits(False)
    assert slot() == off
    assert ctx.fetch_ft8_decode(ch) is None and ctx.fetch_ft8_softbits(ch) is None


def test_errors(xctx):
    from cwsl_digi_amd.api import CwslGpuError
    ctx = xctx
    ARG, MODE = -6, -5

    def raises(status, fn, *a):
        with pytest.raises(CwslGpuError) as e:
            fn(*a)
        assert e.value.status == status

    llr = C.metric_sets(C.SEEDS[0])[0]
    raises(ARG, ctx.ldpc_decode, llr, 30)                              # no code loaded
    raises(ARG, ctx.enable_ft8_decode, True, 30, 7)                    # no code, no sync, no soft bits
    ctx.enable_ft8_decode(False)                                       # switching it off is always allowed
    ctx.set_ldpc_code(C.make_code(C.SEEDS[0])["nm"])
    raises(ARG, ctx.enable_ft8_decode, True, 30, 7)                    # a code, but no sync stage
    ctx.enable_sync(True, 1.5, 200, 200, 3000)
    raises(ARG, ctx.enable_ft8_decode, True, 30, 7)                    # ... and no soft bits
    ctx.enable_ft8_softbits(True)
    for mi, ns in ((0, 7), (201, 7), (30, -1), (30, 23)):
        raises(ARG, ctx.enable_ft8_decode, True, mi, ns)
    ctx.enable_ft8_decode(True, 200, 22)
    ctx.enable_ft8_decode(True, 1, 0)
    # each kind of bad table is rejected and the code loaded before stays in force
    want = C.reference_records(C.SEEDS[0], 30)
    for kind in C.BAD_TABLES:
        raises(ARG, ctx.set_ldpc_code, C.bad_table(C.SEEDS[1], kind))
        _same(ctx.ldpc_decode(llr, 30), want)
    raises(ARG, ctx.ldpc_decode, llr, 0)
    raises(ARG, ctx.ldpc_decode, llr, 201)
    # a fetch on an FT4 channel; a fetch before any frame
    rx = ctx.receiver_open(FS, BLK, 0)
    c4, c8 = ctx.channel_open(rx, 3000, "FT4"), ctx.channel_open(rx, -3000, "FT8")
    raises(MODE, ctx.fetch_ft8_decode, c4)
    assert ctx.fetch_ft8_decode(c8) is None
