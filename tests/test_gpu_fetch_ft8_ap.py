"""GPU: cwslg_fetch_ft8_ap -- the a-priori words of the FT8 group in one fetch (include/cwsl_gpu.h, "FT8 a-priori decoding";
csrc/ap_kernels.hpp behind csrc/harvest_kernels.hpp).  Every comparison is byte for byte: against tests/ap_ref.py + tests/decodes_ref.py applied
to the GPU's OWN lists, soft, decode and OSD records of the slot of tests/ap_cases.py (tests/test_ap_inputs.py proves on the CPU chain what that
slot contains).  The call changes nothing: the other fetches of the epoch return the same bytes before and after it."""
import ctypes as CT

import numpy as np
import pytest

import ap_cases as C
import ap_ref as AP
import decodes_ref as DR
import ldpc_cases as LC
import record_race_cases as RC

pytestmark = pytest.mark.gpu
NO_FRAME, ARG = -9, -6
BIG = 1 << 16
CODE = LC.make_code(C.SEED)["code"]


@pytest.fixture
def xctx():
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


class _Slot:
    """n_chan FT8 channels on one receiver with the whole chain on, the first (discarding) boundary fired, then the slot and its boundary."""

    def __init__(self, ctx, n_chan, max_cand, osd=True, n_pat=2):
        self.ctx = ctx
        ctx.enable_sync(True, C.SLOT_SYNC["syncmin"], max_cand, C.SLOT_SYNC["f_lo"], C.SLOT_SYNC["f_hi"])
        ctx.set_ldpc_code(LC.make_code(C.SEED)["nm"])
        ctx.enable_ft8_softbits(True)
        ctx.enable_ft8_decode(True, *RC.DECODE8)
        ctx.enable_ft8_osd(osd, *RC.OSD8)
        if n_pat:
            ctx.set_ft8_ap(C.slot_patterns(n_pat), C.MAX_ITER, C.SLOT_MIN_NSYNC)
        self.rx = ctx.receiver_open(C.FS, C.BLK8, 0)
        self.chans = [ctx.channel_open(self.rx, rf, "FT8") for rf in C.SLOT_RF[:n_chan]]
        ctx.slot_boundary("FT8", C.start_epoch(0))
        self.push()
        ctx.slot_boundary("FT8", C.start_epoch(1))

    def push(self):
        iq, step = C.slot_iq(), 64 * C.BLK8
        for k in range(0, len(iq), step):
            self.ctx.push_iq(self.rx, iq[k:k + step])

    def expected(self, n_pat=2, max_out=None):
        """ap_ref + decodes_ref on the GPU's own records of the channels whose decode records are of the slot's epoch."""
        E, inp = C.start_epoch(0), []
        for ch in self.chans:
            lst = self.ctx.fetch_candidates(ch, 600, with_epoch=True)
            soft = self.ctx.fetch_ft8_softbits(ch, 600, with_epoch=True)
            msg = self.ctx.fetch_ft8_decode(ch, 600, with_epoch=True)
            osd = self.ctx.fetch_ft8_osd(ch, 600, with_epoch=True)
            if msg is None or msg[1] != E:
                continue
            assert lst[1] == E and soft[3] == E
            o = osd[0] if osd is not None and osd[1] == E else None
            llr, nsync = soft[0], soft[2]
            gate = AP.fetch_gate(msg[0], o, nsync, C.SLOT_MIN_NSYNC)
            ap = AP.decode(CODE, llr, C.slot_patterns(n_pat), C.MAX_ITER, gate) if len(llr) else np.zeros(0, AP.AP_MSG_DTYPE)
            inp.append((ch, DR.where_ft8(lst[0]), ap))
        return C.ap_decodes(inp, max_out) + (len(inp),)

    def others(self):
        """What the other fetches of the epoch hand out, as bytes."""
        d, r = self.ctx.fetch_decodes("FT8", 0, BIG), self.ctx.fetch_decode_reports("FT8", 0, BIG)
        per = [(repr(self.ctx.fetch_candidates(ch, 600, with_epoch=True)), self.ctx.fetch_ft8_decode(ch, 600).tobytes(),
                None if self.ctx.fetch_ft8_osd(ch, 600) is None else self.ctx.fetch_ft8_osd(ch, 600).tobytes()) for ch in self.chans]
        return (d[0].tobytes(), d[1:], r[0].tobytes(), r[1].tobytes(), r[2:], per)


def _same(got, want):
    assert got.dtype == DR.DECODE_DTYPE and got.tobytes() == want.tobytes(), (len(got), len(want), got[:4], want[:4])


@pytest.mark.parametrize("max_cand", [1, 5, 100])
@pytest.mark.parametrize("osd", [True, False], ids=["osd", "no_osd"])
@pytest.mark.parametrize("n_chan", [1, 2, 5])
def test_against_own_records(xctx, n_chan, osd, max_cand):
    """1, 2 and 5 channels (the last three hear noise: a run of channels without finds), OSD on or off at the boundary (the gate changes), the
    list cut at 1, 5 and 100: records, order, n_total, n_channels and the epoch; the same bytes on a second call, with the explicit epoch; the
    other fetches of the epoch and stats.sync_launches untouched."""
    s = _Slot(xctx, n_chan, max_cand, osd=osd)
    E = C.start_epoch(0)
    before, launches = s.others(), xctx.stats()["sync_launches"]
    want, total, n_part = s.expected()
    got, e, n_total, n_ch = xctx.fetch_ft8_ap(0, BIG)
    assert (e, n_total, n_ch) == (E, total, n_part) and n_part == n_chan, (e, n_total, n_ch, total, n_part)
    _same(got, want)
    again = xctx.fetch_ft8_ap(E, BIG)
    assert again[1:] == (E, n_total, n_ch) and again[0].tobytes() == got.tobytes()
    assert s.others() == before and xctx.stats()["sync_launches"] == launches
    assert xctx.fetch_ft8_ap(E + 15, BIG) is None                       # an epoch no channel has
    if max_cand == 100:
        words = [g["bits"].tobytes() for g in got if g["ch_id"] == s.chans[0]]
        assert (got["by_osd"] == 2).all() and C.bits12(C.MSG_A) in words and C.bits12(C.MSG_E) in words
        assert got["ndup"].max() == 2 and set(got["set"]) == {0, 1} and (got["dmin"] > 0).all()
        assert (C.bits12(C.MSG_B) in words) == (not osd)                # the entry OSD decoded is attempted only with OSD off
        assert (got["ch_id"] == s.chans[0]).all()                       # no find on the other channels
        from cwsl_digi_amd.api import merge_ap_decodes
        dec = xctx.fetch_decodes("FT8", E, BIG)[0]
        merged = merge_ap_decodes(dec, got)
        have = {d["bits"].tobytes() for d in dec}
        assert len(merged) == len(dec) + sum(1 for w in words if w not in have) < len(dec) + len(got)


def _raw(ctx, E, dst, mx, with_channels=True):
    t0, n, nt, nc = CT.c_uint64(E), CT.c_int(-1), CT.c_int(-1), CT.c_int(-1)
    rc = ctx.L.cwslg_fetch_ft8_ap(ctx.h, CT.byref(t0), None if dst is None else dst.ctypes.data, mx, CT.byref(n), CT.byref(nt),
                                  CT.byref(nc) if with_channels else None)
    return rc, t0.value, n.value, nt.value, nc.value


def test_truncation_by_max(xctx):
    """max = 0, 1, n_total - 1, n_total, n_total + 1, and dst null with max 0: n = min(n_total, max), the first n records of the full answer,
    n_total whole, and not a byte written beyond record n."""
    s = _Slot(xctx, 2, 100)
    full, total, _ = s.expected()
    E = C.start_epoch(0)
    assert total >= 3
    for mx in (0, 1, total - 1, total, total + 1):
        dst = np.full(total + 2, 0xAB, np.uint8).repeat(40).view(DR.DECODE_DTYPE)
        rc, e, n, nt, nc = _raw(xctx, 0, dst, mx)
        assert (rc, e, n, nt, nc) == (0, E, min(total, mx), total, 2), (mx, rc, e, n, nt, nc)
        assert dst[:n].tobytes() == full[:n].tobytes()
        assert set(dst[n:].tobytes()) == {0xAB}
    assert _raw(xctx, 0, None, 0) == (0, E, 0, total, 2)
    assert _raw(xctx, E, None, 0, with_channels=False)[:4] == (0, E, 0, total)


def test_patterns_in_force_at_the_call_and_a_boundary_with_the_decode_off(xctx):
    """Other patterns between two calls on one epoch: each call answers for the patterns in force when it is made.  Then a boundary with the decode
    off: nothing to fetch, never the older slot's words under a newer epoch."""
    s = _Slot(xctx, 2, 100)
    first = xctx.fetch_ft8_ap(0, BIG)
    _same(first[0], s.expected(2)[0])
    xctx.set_ft8_ap(C.slot_patterns(1), C.MAX_ITER, C.SLOT_MIN_NSYNC)
    one = xctx.fetch_ft8_ap(0, BIG)
    _same(one[0], s.expected(1)[0])
    assert 0 < one[2] < first[2] and (one[0]["set"] == 0).all()
    xctx.set_ft8_ap(C.slot_patterns(2), C.MAX_ITER, C.SLOT_MIN_NSYNC)
    assert xctx.fetch_ft8_ap(0, BIG)[0].tobytes() == first[0].tobytes()
    xctx.enable_ft8_decode(False, *RC.DECODE8)
    s.push()
    xctx.slot_boundary("FT8", C.start_epoch(2))
    assert xctx.fetch_ft8_ap(0, BIG) is None and _raw(xctx, 0, None, 0) == (NO_FRAME, 0, 0, 0, 0)
    assert _raw(xctx, C.start_epoch(0), None, 0)[0] == NO_FRAME


def test_argument_errors(xctx):
    s = _Slot(xctx, 1, 5, n_pat=0)
    E = C.start_epoch(0)
    dst = np.zeros(4, DR.DECODE_DTYPE)
    assert _raw(xctx, 0, dst, 4) == (ARG, 0, 0, 0, 0)                   # no pattern set
    assert b"pattern" in xctx.L.cwslg_last_error(xctx.h)
    xctx.set_ft8_ap(C.slot_patterns(2), C.MAX_ITER, C.SLOT_MIN_NSYNC)
    assert _raw(xctx, 0, dst, 4)[:2] == (0, E)
    assert _raw(xctx, 0, None, 4)[0] == ARG                             # dst null with max > 0
    t0, n, nt = CT.c_uint64(0), CT.c_int(), CT.c_int()
    f = xctx.L.cwslg_fetch_ft8_ap
    assert f(None, CT.byref(t0), dst.ctypes.data, 4, CT.byref(n), CT.byref(nt), None) == ARG
    assert f(xctx.h, None, dst.ctypes.data, 4, CT.byref(n), CT.byref(nt), None) == ARG
    assert f(xctx.h, CT.byref(t0), dst.ctypes.data, 4, None, CT.byref(nt), None) == ARG
    assert f(xctx.h, CT.byref(t0), dst.ctypes.data, 4, CT.byref(n), None, None) == ARG
    xctx.set_ft8_ap(C.slot_patterns(0), C.MAX_ITER, C.SLOT_MIN_NSYNC)    # cleared again
    assert _raw(xctx, 0, dst, 4)[0] == ARG


def test_an_ft4_only_context_has_nothing_to_fetch(xctx):
    """The call is the FT8 group's: a context whose only channels are FT4 ones answers CWSLG_ERR_NO_FRAME, whatever the FT4 chain holds."""
    xctx.set_ldpc_code(LC.make_code(C.SEED)["nm"])
    xctx.set_ft8_ap(C.slot_patterns(2), C.MAX_ITER, C.SLOT_MIN_NSYNC)
    rx = xctx.receiver_open(C.FS, RC.BLK["FT4"], 0)
    xctx.channel_open(rx, 0, "FT4")
    assert _raw(xctx, 0, None, 0) == (NO_FRAME, 0, 0, 0, 0)
