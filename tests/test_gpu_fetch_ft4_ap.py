"""GPU: cwslg_fetch_ft4_ap -- the a-priori words of the FT4 group in one fetch (include/cwsl_gpu.h, "FT4 a-priori decoding"; the FT4 addressing
of csrc/ap_kernels.hpp behind csrc/harvest_kernels.hpp's FT4 modes).  Every comparison is byte for byte: against tests/ft4_ap_ref.py +
tests/decodes_ref.py applied to the GPU's OWN sync, soft, decode and OSD records of the epoch, on the two slots of tests/ft4_ap_cases.py
(tests/test_ft4_ap_inputs.py proves on the CPU chain what they contain).  The call changes nothing: the other fetches of the epoch return the
same bytes before and after it."""
import ctypes as CT

import numpy as np
import pytest

import ap_cases as APC
import decodes_ref as DR
import ft4_ap_cases as F
import ft4_ap_ref as A4
import ft4_decode_cases as D
import ldpc_cases as LC
import record_race_cases as RC

pytestmark = pytest.mark.gpu
NO_FRAME, ARG = -9, -6
BIG = 1 << 16
MODE = "FT4"
CODE = LC.make_code(F.SEED)["code"]
_AP_CACHE = {}


@pytest.fixture
def xctx():
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


def _ap_of(soft, msg, osd, pats, mins):
    """ft4_ap_ref.decode, computed once per distinct input: the same channel's records come back in several tests."""
    key = (soft["llr"].tobytes(), np.asarray(soft["nsync"]).tobytes(), np.asarray(soft["nqual"]).tobytes(), msg.tobytes(),
           None if osd is None else osd.tobytes(), pats.tobytes(), mins)
    if key not in _AP_CACHE:
        _AP_CACHE[key] = A4.decode(CODE, soft, msg, osd, pats, F.AP_MAX_ITER, *mins)
    return _AP_CACHE[key]


class _Slot:
    """n_chan FT4 channels on one receiver with the slot's chain on, the first (discarding) boundary fired, then the slot and its boundary."""

    def __init__(self, ctx, slot, n_chan, max_cand, osd=None, n_pat=None, set_patterns=True, syncmin8=RC.SYNC["syncmin"]):
        self.ctx, self.slot = ctx, slot
        dec, osd_cfg, self.mins = F.SETTINGS[slot]
        self.osd = (osd_cfg is not None) if osd is None else osd
        s = RC.SYNC
        ctx.enable_sync(True, syncmin8, max_cand, s["f_lo"], s["f_hi"])      # (the FT8 threshold; FT4 has its own, below)
        ctx.set_ft4_syncmin(F.SYNCMIN)
        ctx.set_ldpc_code(LC.make_code(F.SEED)["nm"])
        ctx.enable_ft4_softbits(True)
        ctx.enable_ft4_decode(True, *dec)
        ctx.enable_ft4_osd(self.osd, *(osd_cfg or RC.OSD4))
        if set_patterns:
            self.set_patterns(n_pat)
        self.rx = ctx.receiver_open(F.FS, F.BLK, 0)
        self.chans = [ctx.channel_open(self.rx, rf, MODE) for rf in F.RF[:n_chan]]
        ctx.slot_boundary(MODE, F.start_epoch(0))
        self.push()
        ctx.slot_boundary(MODE, F.start_epoch(1))

    def set_patterns(self, n_pat=None):
        self.ctx.set_ft4_ap(F.patterns(self.slot, n_pat), F.AP_MAX_ITER, *self.mins)

    def push(self):
        iq, step = F.slot_iq(self.slot), 64 * F.BLK
        for k in range(0, len(iq), step):
            self.ctx.push_iq(self.rx, iq[k:k + step])

    def expected(self, n_pat=None, max_out=None):
        """ft4_ap_ref + decodes_ref on the GPU's own records of the channels whose decode records are of the slot's epoch."""
        E, inp = F.start_epoch(0), []
        for ch in self.chans:
            msg = self.ctx.fetch_ft4_decode(ch, 1800, with_epoch=True)
            if msg is None or msg[1] != E:
                continue
            sync = self.ctx.fetch_ft4_sync(ch, 1800, with_epoch=True)
            soft = self.ctx.fetch_ft4_softbits(ch, 1800, with_epoch=True)
            osd = self.ctx.fetch_ft4_osd(ch, 1800, with_epoch=True)
            assert sync[1] == E and soft[4] == E and len(sync[0]) == len(msg[0]) == len(soft[0])
            o = osd[0] if osd is not None and osd[1] == E else None
            assert (o is not None) == self.osd
            ap = _ap_of(D.soft_dict(*soft[:4]), msg[0], o, F.patterns(self.slot, n_pat), self.mins)
            inp.append((ch, DR.where_ft4(sync[0]), ap))
        return A4.ap_decodes(inp, max_out) + (len(inp),)

    def others(self):
        """What the other fetches of the epoch hand out, as bytes."""
        c = self.ctx
        d, r = c.fetch_decodes(MODE, 0, BIG), c.fetch_ft4_decode_reports(0, BIG)
        per = [(repr(c.fetch_ft4_sync(ch, 1800, with_epoch=True)), c.fetch_ft4_softbits(ch, 1800)[0].tobytes(), c.fetch_ft4_decode(ch, 1800).tobytes(),
                None if c.fetch_ft4_osd(ch, 1800) is None else c.fetch_ft4_osd(ch, 1800).tobytes()) for ch in self.chans]
        return (d[0].tobytes(), d[1:], r[0].tobytes(), r[1].tobytes(), r[2:], per)


def _same(got, want):
    assert got.dtype == DR.DECODE_DTYPE and got.tobytes() == want.tobytes(), (len(got), len(want), got[:4], want[:4])


def _check_call(ctx, s, n_chan):
    """One call against the restatement, a second call, the explicit epoch, an epoch no channel has; the other fetches untouched."""
    E = F.start_epoch(0)
    before, launches = s.others(), ctx.stats()["sync_launches"]
    want, total, n_part = s.expected()
    got, e, n_total, n_ch = ctx.fetch_ft4_ap(0, BIG)
    assert (e, n_total, n_ch) == (E, total, n_part) and n_part == n_chan, (e, n_total, n_ch, total, n_part)
    _same(got, want)
    again = ctx.fetch_ft4_ap(E, BIG)
    assert again[1:] == (E, n_total, n_ch) and again[0].tobytes() == got.tobytes()
    assert s.others() == before and ctx.stats()["sync_launches"] == launches
    assert ctx.fetch_ft4_ap(E + 7, BIG) is None
    assert (got["by_osd"] == 2).all()
    return got


@pytest.mark.parametrize("max_cand", [1, 4, 30])
@pytest.mark.parametrize("n_chan", [1, 2, 3])
@pytest.mark.parametrize("slot", F.SLOTS)
def test_against_own_records(xctx, slot, n_chan, max_cand):
    """Both slots at 1, 2 and 3 channels (the third hears noise: a channel without finds behind channels with them), the list cut at 1, 4 and 30
    (the cut falls inside a candidate's records): records, order, n_total, n_channels and the epoch."""
    s = _Slot(xctx, slot, n_chan, max_cand)
    got = _check_call(xctx, s, n_chan)
    if max_cand == 30 and n_chan == 3:
        st, pt = got["set"] & 3, got["set"] >> 2
        assert set(got["ch_id"]) <= set(s.chans[:2]) and (got["dmin"] > 0).any()
        if slot == "starved":
            # what tests/test_ft4_ap_inputs.py proves of the slot shows here: many finds, later sets, later patterns, one folded pair
            assert len(got) >= 6 and (st != 0).any() and (pt != 0).any() and (got["ndup"] == 2).sum() == 1
            words = {g["bits"].tobytes() for g in got}
            assert words <= set(F.sent(slot, 0) + F.sent(slot, 1))
            dec = xctx.fetch_decodes(MODE, 0, BIG)[0]                   # the records BP did decode are not attempted: their words are not among the finds
            assert len(dec) >= 1 and not ({d["bits"].tobytes() for d in dec} & words)
        else:
            assert len(got) >= 1 and set(pt) == {0, 1}
            from cwsl_digi_amd.api import merge_ap_decodes, ap_set_split
            dec = xctx.fetch_decodes(MODE, 0, BIG)[0]
            merged = merge_ap_decodes(dec, got)
            assert len(merged) == len(dec) + len(got) and set(merged["by_osd"]) == {0, 1, 2}
            assert [ap_set_split(int(v)) for v in got["set"]] == [A4.split(v) for v in got["set"]]


@pytest.mark.parametrize("slot", F.SLOTS)
def test_the_osd_switch_at_the_boundary_changes_the_gate(xctx, slot):
    """The starved slot with OSD on at the boundary (OSD returns the words BP was starved of: those records are no longer taken), the normal slot
    with OSD off (the records OSD decoded are attempted, and found)."""
    natural = F.SETTINGS[slot][1] is not None
    s = _Slot(xctx, slot, 3, 30, osd=not natural)
    got = _check_call(xctx, s, 3)
    ref_total = F.expected(slot)[1]                                      # the CPU chain's count under the slot's own switch
    assert len(got) > ref_total if natural else len(got) < ref_total


def _raw(ctx, E, dst, mx, with_channels=True):
    t0, n, nt, nc = CT.c_uint64(E), CT.c_int(-1), CT.c_int(-1), CT.c_int(-1)
    rc = ctx.L.cwslg_fetch_ft4_ap(ctx.h, CT.byref(t0), None if dst is None else dst.ctypes.data, mx, CT.byref(n), CT.byref(nt),
                                  CT.byref(nc) if with_channels else None)
    return rc, t0.value, n.value, nt.value, nc.value


def test_truncation_by_max(xctx):
    """max = 0, 1, n_total - 1, n_total, n_total + 1, and dst null with max 0: n = min(n_total, max), the first n records of the full answer,
    n_total whole, and not a byte written beyond record n."""
    s = _Slot(xctx, "starved", 2, 30)
    full, total, _ = s.expected()
    E = F.start_epoch(0)
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
    """1 and 3 patterns between calls on one epoch: each call answers for the patterns in force when it is made.  Then a boundary with the FT4
    decode off: nothing to fetch, never the older slot's words under a newer epoch."""
    s = _Slot(xctx, "starved", 2, 30)
    first = xctx.fetch_ft4_ap(0, BIG)
    _same(first[0], s.expected()[0])
    s.set_patterns(1)
    one = xctx.fetch_ft4_ap(0, BIG)
    _same(one[0], s.expected(1)[0])
    assert one[2] > 0 and (one[0]["set"] >> 2 == 0).all() and one[0].tobytes() != first[0].tobytes()
    s.set_patterns()
    assert xctx.fetch_ft4_ap(0, BIG)[0].tobytes() == first[0].tobytes()
    xctx.enable_ft4_decode(False, *F.SETTINGS["starved"][0])
    s.push()
    xctx.slot_boundary(MODE, F.start_epoch(2))
    assert xctx.fetch_ft4_ap(0, BIG) is None and _raw(xctx, 0, None, 0) == (NO_FRAME, 0, 0, 0, 0)
    assert _raw(xctx, F.start_epoch(0), None, 0)[0] == NO_FRAME


def test_one_pattern_on_the_normal_slot(xctx):
    s = _Slot(xctx, "normal", 3, 30, n_pat=1)
    want, total, n_part = s.expected(1)
    got = xctx.fetch_ft4_ap(0, BIG)
    assert got[1:] == (F.start_epoch(0), total, 3) and total >= 1
    _same(got[0], want)
    assert (got[0]["set"] >> 2 == 0).all()


def test_argument_errors(xctx):
    s = _Slot(xctx, "normal", 1, 4, set_patterns=False)
    E = F.start_epoch(0)
    dst = np.zeros(4, DR.DECODE_DTYPE)
    assert _raw(xctx, 0, dst, 4) == (ARG, 0, 0, 0, 0)                   # no FT4 pattern set
    assert b"pattern" in xctx.L.cwslg_last_error(xctx.h)
    xctx.set_ft8_ap(APC.slot_patterns(2), 30, 7)                        # the FT8 patterns are another state: still none for FT4
    assert _raw(xctx, 0, dst, 4)[0] == ARG
    s.set_patterns()
    assert _raw(xctx, 0, dst, 4)[:2] == (0, E)
    assert _raw(xctx, 0, None, 4)[0] == ARG                             # dst null with max > 0
    t0, n, nt = CT.c_uint64(0), CT.c_int(), CT.c_int()
    f = xctx.L.cwslg_fetch_ft4_ap
    assert f(None, CT.byref(t0), dst.ctypes.data, 4, CT.byref(n), CT.byref(nt), None) == ARG
    assert f(xctx.h, None, dst.ctypes.data, 4, CT.byref(n), CT.byref(nt), None) == ARG
    assert f(xctx.h, CT.byref(t0), dst.ctypes.data, 4, None, CT.byref(nt), None) == ARG
    assert f(xctx.h, CT.byref(t0), dst.ctypes.data, 4, CT.byref(n), None, None) == ARG
    # the setter: ranges and pattern errors leave the patterns in force
    before = xctx.fetch_ft4_ap(0, BIG)[0].tobytes()
    pat = F.patterns("normal")
    g = xctx.L.cwslg_set_ft4_ap
    for args in ((0, 8, 20), (201, 8, 20), (30, -1, 20), (30, 18, 20), (30, 8, -1), (30, 8, 34)):
        assert g(xctx.h, pat.ctypes.data, len(pat), *args) == ARG, args
    assert g(None, pat.ctypes.data, len(pat), 30, 8, 20) == ARG and g(xctx.h, pat.ctypes.data, 9, 30, 8, 20) == ARG
    assert g(xctx.h, None, 1, 30, 8, 20) == ARG
    bad = pat.copy()
    bad["mask"][1, 11] |= 0x10
    assert g(xctx.h, bad.ctypes.data, len(bad), 30, 8, 20) == ARG
    bad = pat.copy()
    bad["mask"][0, 0] &= 0x7f
    bad["value"][0, 0] |= 0x80
    assert g(xctx.h, bad.ctypes.data, len(bad), 30, 8, 20) == ARG
    assert xctx.fetch_ft4_ap(0, BIG)[0].tobytes() == before
    for mins in ((17, 0), (0, 33)):                                      # in range, and nothing is attempted
        assert g(xctx.h, pat.ctypes.data, len(pat), 30, *mins) == 0
        assert xctx.fetch_ft4_ap(0, BIG)[1:] == (E, 0, 1)
    s.set_patterns(0)                                                    # cleared again
    assert _raw(xctx, 0, dst, 4)[0] == ARG


def test_the_ft8_call_on_the_same_context_is_untouched(xctx):
    """An FT8 channel (tests/ap_cases.py's slot, its own patterns) and the FT4 channels in one context: cwslg_fetch_ft8_ap returns the same bytes
    before and after the FT4 call and after other FT4 patterns are set, and the FT4 call is not moved by the FT8 patterns."""
    s = _Slot(xctx, "normal", 2, 30, syncmin8=APC.SLOT_SYNC["syncmin"])
    xctx.enable_ft8_softbits(True)
    xctx.enable_ft8_decode(True, *RC.DECODE8)
    xctx.enable_ft8_osd(True, *RC.OSD8)
    xctx.set_ft8_ap(APC.slot_patterns(2), APC.MAX_ITER, APC.SLOT_MIN_NSYNC)
    rx8 = xctx.receiver_open(APC.FS, APC.BLK8, 0)
    xctx.channel_open(rx8, APC.SLOT_RF[0], "FT8")
    xctx.slot_boundary("FT8", APC.start_epoch(0))
    iq, step = APC.slot_iq(), 64 * APC.BLK8
    for k in range(0, len(iq), step):
        xctx.push_iq(rx8, iq[k:k + step])
    xctx.slot_boundary("FT8", APC.start_epoch(1))
    ft8 = xctx.fetch_ft8_ap(0, BIG)
    assert ft8 is not None and ft8[1] == APC.start_epoch(0) and ft8[2] >= 1
    ft4 = xctx.fetch_ft4_ap(0, BIG)
    _same(ft4[0], s.expected()[0])
    assert ft4[1] == F.start_epoch(0) and ft4[3] == 2
    again8 = xctx.fetch_ft8_ap(0, BIG)
    assert again8[1:] == ft8[1:] and again8[0].tobytes() == ft8[0].tobytes()
    s.set_patterns(1)
    xctx.set_ft8_ap(APC.slot_patterns(1), APC.MAX_ITER, APC.SLOT_MIN_NSYNC)
    s.set_patterns()
    assert xctx.fetch_ft4_ap(0, BIG)[0].tobytes() == ft4[0].tobytes()   # FT8's patterns changed: the FT4 answer has not
    xctx.set_ft8_ap(APC.slot_patterns(2), APC.MAX_ITER, APC.SLOT_MIN_NSYNC)
    assert xctx.fetch_ft8_ap(0, BIG)[0].tobytes() == ft8[0].tobytes()
