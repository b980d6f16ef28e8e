"""GPU: cwslg_fetch_decode_reports -- cwslg_fetch_decodes with a signal report per decode, made on the device (include/cwsl_gpu.h, "FT8 signal
reports"; decode_report_kernel of csrc/harvest_kernels.hpp).  Every comparison is byte for byte: `dec` against cwslg_fetch_decodes, `rep`
against tests/decode_reports_ref.py applied to the GPU's own plane (cwslg_sync_debug_fetch what 0), list and decodes; nsync against the soft
record's.  The slots are tests/decode_report_cases.py's (tests/test_decode_reports_inputs.py proves what they contain)."""
import ctypes as C

import numpy as np
import pytest

import decode_report_cases as RC8
import decode_reports_ref as RR
import decodes_ref as DR
import harvest_cases as H
import ldpc_cases as LC
import record_race_cases as RC
import report_kernel_cases as K

pytestmark = pytest.mark.gpu
NO_FRAME, ERR_ARG = -9, -6
BIG = 1 << 16
MODE = "FT8"


@pytest.fixture
def xctx():
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


class _Group:
    """The FT8 receiver and channels of decode_report_cases, everything on, the first (discarding) boundary fired."""

    def __init__(self, ctx, rfs, max_cand, osd=True, syncmin=None, fire=True, seed=RC8.SEED):
        self.ctx = ctx
        s = RC8.SYNC8
        ctx.enable_sync(True, s["syncmin"] if syncmin is None else syncmin, max_cand, s["f_lo"], s["f_hi"])
        ctx.set_ldpc_code(LC.make_code(seed)["nm"])
        self.stages(osd=osd)
        self.rx = ctx.receiver_open(RC8.FS, RC8.BLK, 0)
        self.chans = [ctx.channel_open(self.rx, rf, MODE) for rf in rfs]
        if fire:
            ctx.slot_boundary(MODE, RC8.start_epoch(0))

    def stages(self, soft=True, decode=True, osd=True):
        self.ctx.enable_ft8_softbits(soft)
        self.ctx.enable_ft8_decode(decode, *RC.DECODE8)
        self.ctx.enable_ft8_osd(osd, *RC.OSD8)

    def push(self, e):
        iq, step = RC8.slot_iq(e), 64 * RC8.BLK
        for k in range(0, len(iq), step):
            self.ctx.push_iq(self.rx, iq[k:k + step])

    def slot(self, e):
        self.push(e)
        self.ctx.slot_boundary(MODE, RC8.start_epoch(e + 1))


def _plane(ctx, ch):
    pl = ctx.sync_debug(ch, "spectra")
    assert pl.dtype == np.float32 and pl.ndim == 2 and pl.shape[0] == 372
    return pl


def _want(ctx, dec, seed=RC8.SEED):
    """decode_reports_ref on the GPU's own planes and lists of the channels that `dec` names."""
    chans = sorted({int(c) for c in dec["ch_id"]})
    planes = {ch: _plane(ctx, ch) for ch in chans}
    lists = {ch: ctx.fetch_candidates(ch, 600) for ch in chans}
    return RR.reports(K.encoder(seed), planes, lists, dec)


def _check(ctx, E=0, seed=RC8.SEED, max_out=BIG):
    """One call against cwslg_fetch_decodes and the restatement; -> (dec, rep, E, n_total, n_channels)."""
    plain = ctx.fetch_decodes(MODE, E, max_out)
    got = ctx.fetch_decode_reports(MODE, E, max_out)
    assert (plain is None) == (got is None)
    if got is None:
        return None
    dec, rep, E_got, n_total, n_ch = got
    assert (E_got, n_total, n_ch) == plain[1:] and dec.dtype == DR.DECODE_DTYPE and dec.tobytes() == plain[0].tobytes()
    assert rep.dtype == RR.REPORT_DTYPE and len(rep) == len(dec)
    want = _want(ctx, dec, seed)
    bad = [p for p in range(len(dec)) if rep[p].tobytes() != want[p].tobytes()]
    assert not bad, (bad[:5], rep[bad[:3]], want[bad[:3]], dec[bad[:3]])
    return got


def _nsync_equals_the_soft_records(ctx, dec, rep):
    for ch in sorted({int(c) for c in dec["ch_id"]}):
        nsync = np.asarray(ctx.fetch_ft8_softbits(ch, 600)[2])
        sel = dec["ch_id"] == ch
        assert np.array_equal(rep["nsync"][sel], nsync[dec["entry"][sel]])


# ---- the vetted recipe ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_cand", [1, 5, 100])
@pytest.mark.parametrize("osd", [True, False], ids=["osd", "no_osd"])
@pytest.mark.parametrize("n_chan", [1, 2])
def test_reports_against_the_restatement(xctx, n_chan, osd, max_cand):
    g = _Group(xctx, RC8.RF[:n_chan], max_cand, osd=osd)
    assert xctx.fetch_decode_reports(MODE) is None                      # the first boundary discards: nothing yet
    seen = np.zeros(0, RR.REPORT_DTYPE)
    for e in range(RC8.N_EPOCHS):
        g.slot(e)
        dec, rep, E, n_total, n_ch = _check(xctx)
        assert (E, n_ch) == (RC8.start_epoch(e), n_chan) and n_total == len(dec)
        _nsync_equals_the_soft_records(xctx, dec, rep)
        again = xctx.fetch_decode_reports(MODE, E, BIG)                 # two calls on one epoch: the same bytes
        assert again[2:] == (E, n_total, n_ch) and again[0].tobytes() == dec.tobytes() and again[1].tobytes() == rep.tobytes()
        seen = np.concatenate([seen, rep])
    if max_cand == 100 and osd:
        # (the slots do contain what they were made for: test_decode_reports_inputs.py proves it on the CPU chain)
        assert (seen["nsymerr"] == 0).any() and (seen["nsymerr"] > 0).any() and (seen["snr_db"] == -24).any() and (seen["snr_db"] > -24).any()


# ---- truncation ---------------------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, group, E, dec, rep, mx, with_channels=True):
    t0, n, nt, nc = C.c_uint64(E), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = ctx.L.cwslg_fetch_decode_reports(ctx.h, group, C.byref(t0), None if dec is None else dec.ctypes.data, None if rep is None else rep.ctypes.data, mx,
                                          C.byref(n), C.byref(nt), C.byref(nc) if with_channels else None)
    return rc, t0.value, n.value, nt.value, nc.value


def test_truncation_by_max(xctx):
    """max = 0, 1, n_total - 1, n_total, n_total + 1; a null dec or a null rep: n = min(n_total, max), the first n of the full answer, and not a byte
    written beyond record n of either block."""
    import cwsl_digi_amd as P
    g = _Group(xctx, RC8.RF, 100)
    g.slot(0)
    full_dec, full_rep, E0, total, _ = _check(xctx)
    assert total >= 3
    grp = P.GROUPS[MODE]
    for mx in (0, 1, total - 1, total, total + 1):
        for null in ("", "dec", "rep"):
            dec = None if null == "dec" else np.full(total + 2, 0xAB, np.uint8).repeat(40).view(DR.DECODE_DTYPE)
            rep = None if null == "rep" else np.full(total + 2, 0xAB, np.uint8).repeat(16).view(RR.REPORT_DTYPE)
            rc, E, n, nt, nc = _raw(xctx, grp, 0, dec, rep, mx)
            assert (rc, E, n, nt, nc) == (0, E0, min(total, mx), total, 2), (mx, null, rc, E, n, nt, nc)
            if dec is not None:
                assert dec[:n].tobytes() == full_dec[:n].tobytes() and set(dec[n:].tobytes()) == {0xAB}
            if rep is not None:
                assert rep[:n].tobytes() == full_rep[:n].tobytes() and set(rep[n:].tobytes()) == {0xAB}
    assert _raw(xctx, grp, 0, None, None, 5) == (0, E0, min(total, 5), total, 2)
    assert _raw(xctx, grp, 0, None, None, 0, with_channels=False)[:4] == (0, E0, 0, total)


# ---- many channels --------------------------------------------------------------------------------------------------------------------------------------
def _own_bytes(ctx, chans):
    out = []
    for ch in chans:
        try:
            lst = ctx.fetch_candidates(ch, 600, with_epoch=True)
        except Exception:
            lst = None
        soft, msg, osd = (f(ch, 600, with_epoch=True) for f in (ctx.fetch_ft8_softbits, ctx.fetch_ft8_decode, ctx.fetch_ft8_osd))
        out.append((repr(lst), None if soft is None else tuple(np.asarray(a).tobytes() for a in soft[:-1]) + (soft[-1],),
                    None if msg is None else (msg[0].tobytes(), msg[1]), None if osd is None else (osd[0].tobytes(), osd[1])))
    return out


@pytest.mark.parametrize("n_chan", [3, 5, 257])
def test_many_channels(xctx, n_chan):
    """3, 5 and 257 FT8 channels on one receiver, list limit 8, syncmin 2.0: the channels whose passband holds the transmissions decode them, the
    others hear noise and most have an empty list -- runs of channels without decodes, so the offsets search crosses equal offsets and (257) the
    scan's carry.  The per-channel fetches return the same bytes before and after the call; stats.sync_launches does not move."""
    lo, hi = -17400, -13000
    rfs = [RC8.RF[0], RC8.RF[1], 6000][:min(n_chan, 3)] + [int(round(lo + (hi - lo) * j / max(n_chan - 4, 1))) for j in range(n_chan - 3)]
    g = _Group(xctx, rfs, 8, syncmin=2.0)
    g.push(1)
    xctx.slot_boundary(MODE, RC8.start_epoch(1))
    before = _own_bytes(xctx, g.chans)
    launches = xctx.stats()["sync_launches"]
    got = xctx.fetch_decode_reports(MODE, 0, BIG)
    assert xctx.stats()["sync_launches"] == launches
    assert _own_bytes(xctx, g.chans) == before
    dec, rep, E, n_total, n_ch = _check(xctx)
    assert got[0].tobytes() == dec.tobytes() and got[1].tobytes() == rep.tobytes()
    assert n_ch == n_chan and n_total >= 3 and len(set(dec["ch_id"])) >= (1 if n_chan == 3 else 2)
    with_decodes = set(int(c) for c in dec["ch_id"])
    assert any(ch not in with_decodes for ch in g.chans)                # channels without decodes: equal offsets
    _nsync_equals_the_soft_records(xctx, dec, rep)
    cut = xctx.fetch_decode_reports(MODE, E, n_total - 1)
    assert cut[2:] == (E, n_total, n_chan) and cut[0].tobytes() == dec[:-1].tobytes() and cut[1].tobytes() == rep[:-1].tobytes()


# ---- epochs ------------------------------------------------------------------------------------------------------------------------------------------------
def test_epochs_and_switches(xctx):
    """Explicit E, 0 = newest, a stale E; after a boundary with the decode off nothing to fetch; after one with OSD off BP words only."""
    g = _Group(xctx, RC8.RF, RC.MAX_CAND)
    g.slot(0)
    E0, E1, E2 = (RC8.start_epoch(e) for e in range(3))
    for ask in (0, E0):
        assert _check(xctx, ask)[2] == E0
    assert xctx.fetch_decode_reports(MODE, E1, BIG) is None and xctx.fetch_decode_reports(MODE, E0 + 1, BIG) is None
    g.stages(decode=False)
    g.slot(1)
    assert all(xctx.fetch_decode_reports(MODE, ask, BIG) is None for ask in (0, E0, E1))
    g.stages(osd=False)
    g.slot(2)
    dec, rep, E, n_total, n_ch = _check(xctx)
    assert (E, n_ch) == (E2, 2) and not dec["by_osd"].any() and n_total > 0
    assert xctx.fetch_decode_reports(MODE, E1, BIG) is None


def test_one_channel_advanced_alone(xctx):
    g = _Group(xctx, RC8.RF, 100, fire=False)
    js8 = xctx.channel_open(g.rx, RC8.RF[0], "JS8")
    xctx.slot_boundary(MODE, RC8.start_epoch(0))
    g.slot(0)
    late = xctx.channel_open(g.rx, RC8.RF[0] + 100, MODE)
    E0, E1 = RC8.start_epoch(0), RC8.start_epoch(1)
    dec, rep, E, n_total, n_ch = _check(xctx)
    assert (E, n_ch) == (E0, 2) and js8 not in dec["ch_id"] and late not in dec["ch_id"]
    g.push(1)
    xctx.slot_boundary_channel(g.chans[0], RC8.start_epoch(2))
    dec, rep, E, n_total, n_ch = _check(xctx)
    assert (E, n_ch) == (E1, 1) and set(dec["ch_id"]) <= {g.chans[0]}
    dec, rep, E, n_total, n_ch = _check(xctx, E0)
    assert (E, n_ch) == (E0, 1) and set(dec["ch_id"]) <= {g.chans[1]}
    xctx.channel_close(g.chans[0])
    assert _check(xctx)[2:] == (E0, n_total, 1)
    xctx.channel_close(g.chans[1])
    assert xctx.fetch_decode_reports(MODE, 0, BIG) is None


def test_second_code_and_a_table_without_systematic_form(xctx):
    """The report uses the code in force at the call: after a second cwslg_set_ldpc_code the same words are re-encoded under the new table; a
    table whose columns 91..173 are singular loads (and decodes) but has no reports -- CWSLG_ERR_ARG with a text, the decodes untouched."""
    import cwsl_digi_amd as P
    g = _Group(xctx, RC8.RF, 100)
    g.slot(0)
    dec, rep, E, n_total, n_ch = _check(xctx)
    t0 = xctx.ft8_tones(dec["bits"][0])
    assert np.array_equal(t0, RR.tones(K.encoder(RC8.SEED), dec["bits"][0]))
    xctx.set_ldpc_code(LC.make_code(LC.SEEDS[1])["nm"])
    dec2, rep2, E2, n2, _ = _check(xctx, seed=LC.SEEDS[1])
    assert dec2.tobytes() == dec.tobytes() and (E2, n2) == (E, n_total) and rep2.tobytes() != rep.tobytes()
    assert np.array_equal(xctx.ft8_tones(dec["bits"][0]), RR.tones(K.encoder(LC.SEEDS[1]), dec["bits"][0]))
    xctx.set_ldpc_code(K.singular_table(RC8.SEED))                      # accepted: a code, of rank 83, without a systematic form
    d = np.full(n_total, 0xAB, np.uint8).repeat(40).view(DR.DECODE_DTYPE)
    r = np.full(n_total, 0xAB, np.uint8).repeat(16).view(RR.REPORT_DTYPE)
    rc, _, n, nt, nc = _raw(xctx, P.GROUPS[MODE], 0, d, r, n_total)
    assert (rc, n, nt, nc) == (ERR_ARG, 0, 0, 0) and set(d.tobytes()) == {0xAB} and set(r.tobytes()) == {0xAB}
    assert b"singular" in xctx.L.cwslg_last_error(xctx.h)
    tones = np.zeros(79, np.uint8)
    bits = np.ascontiguousarray(dec["bits"][0])
    assert xctx.L.cwslg_ft8_tones(xctx.h, bits.ctypes.data, tones.ctypes.data) == ERR_ARG and not tones.any()
    plain = xctx.fetch_decodes(MODE, 0, BIG)                            # the decodes themselves are untouched
    assert plain[0].tobytes() == dec.tobytes()
    xctx.set_ldpc_code(LC.make_code(RC8.SEED)["nm"])
    again = xctx.fetch_decode_reports(MODE, 0, BIG)
    assert again[0].tobytes() == dec.tobytes() and again[1].tobytes() == rep.tobytes()


# ---- error paths ----------------------------------------------------------------------------------------------------------------------------------------
def test_error_paths(xctx):
    import cwsl_digi_amd as P
    L, h = xctx.L, xctx.h
    dec, rep = np.zeros(4, DR.DECODE_DTYPE), np.zeros(4, RR.REPORT_DTYPE)
    t0, n, nt, nc = C.c_uint64(0), C.c_int(7), C.c_int(7), C.c_int(7)
    args = lambda: (C.byref(t0), dec.ctypes.data, rep.ctypes.data, 4, C.byref(n), C.byref(nt), C.byref(nc))
    xctx.set_ldpc_code(LC.make_code(RC8.SEED)["nm"])
    for group in (-1, P.GROUPS["FT4"], P.GROUPS["Q65_30"], P.GROUPS["S120"], 8):
        assert L.cwslg_fetch_decode_reports(h, group, *args()) == ERR_ARG
    assert L.cwslg_fetch_decode_reports(None, 0, *args()) == ERR_ARG
    assert L.cwslg_fetch_decode_reports(h, 0, None, dec.ctypes.data, rep.ctypes.data, 4, C.byref(n), C.byref(nt), C.byref(nc)) == ERR_ARG
    assert L.cwslg_fetch_decode_reports(h, 0, C.byref(t0), dec.ctypes.data, rep.ctypes.data, 4, None, C.byref(nt), C.byref(nc)) == ERR_ARG
    assert L.cwslg_fetch_decode_reports(h, 0, C.byref(t0), dec.ctypes.data, rep.ctypes.data, 4, C.byref(n), None, C.byref(nc)) == ERR_ARG
    n.value = nt.value = nc.value = 7
    assert L.cwslg_fetch_decode_reports(h, 0, *args()) == NO_FRAME and (n.value, nt.value, nc.value, t0.value) == (0, 0, 0, 0)
    tones = np.zeros(79, np.uint8)
    bits = np.zeros(12, np.uint8)
    assert L.cwslg_ft8_tones(None, bits.ctypes.data, tones.ctypes.data) == ERR_ARG
    assert L.cwslg_ft8_tones(h, None, tones.ctypes.data) == ERR_ARG and L.cwslg_ft8_tones(h, bits.ctypes.data, None) == ERR_ARG


def test_no_code_loaded():
    import cwsl_digi_amd as P
    c = P.Context(0)
    try:
        dec, rep = np.zeros(1, DR.DECODE_DTYPE), np.zeros(1, RR.REPORT_DTYPE)
        t0, n, nt = C.c_uint64(0), C.c_int(7), C.c_int(7)
        assert c.L.cwslg_fetch_decode_reports(c.h, 0, C.byref(t0), dec.ctypes.data, rep.ctypes.data, 1, C.byref(n), C.byref(nt), None) == ERR_ARG
        tones, bits = np.zeros(79, np.uint8), np.zeros(12, np.uint8)
        assert c.L.cwslg_ft8_tones(c.h, bits.ctypes.data, tones.ctypes.data) == ERR_ARG
    finally:
        c.close()
