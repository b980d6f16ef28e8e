"""GPU: cwslg_fetch_ft4_decode_reports -- cwslg_fetch_decodes(FT4) with a signal report per decode, made on the device (include/cwsl_gpu.h, "FT4
signal reports"; ft4_report_kernel of csrc/ft4soft_kernels.hpp).  Every comparison is byte for byte: `dec` against cwslg_fetch_decodes, `rep`
against tests/ft4_decode_reports_ref.py applied to the GPU's own frame spectrum (cwslg_sync_debug_fetch "ft4_cx"), sync records and decodes; nsync
against the soft record's.  The slots are tests/ft4_decode_report_cases.py's (tests/test_ft4_decode_reports_inputs.py proves what they contain)."""
import ctypes as C

import numpy as np
import pytest

import decodes_ref as DR
import ft4_decode_report_cases as RC4
import ft4_decode_reports_ref as R4
import ldpc_cases as LC
import record_race_cases as RC
import report_kernel_cases as K

pytestmark = pytest.mark.gpu
NO_FRAME, ERR_ARG = -9, -6
BIG = 1 << 16
MODE = "FT4"


@pytest.fixture
def xctx():
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


class _Group:
    """The FT4 receiver and channels of ft4_decode_report_cases, everything on, the first (discarding) boundary fired."""

    def __init__(self, ctx, rfs, max_cand, osd=True, fire=True, seed=RC4.SEED):
        self.ctx = ctx
        s = RC.SYNC
        ctx.enable_sync(True, s["syncmin"], max_cand, s["f_lo"], s["f_hi"])
        ctx.set_ft4_syncmin(RC.SYNCMIN_FT4)
        ctx.set_ldpc_code(LC.make_code(seed)["nm"])
        self.stages(osd=osd)
        self.rx = ctx.receiver_open(RC4.FS, RC4.BLK, 0)
        self.chans = [ctx.channel_open(self.rx, rf, MODE) for rf in rfs]
        if fire:
            ctx.slot_boundary(MODE, RC4.start_epoch(0))

    def stages(self, soft=True, decode=True, osd=True):
        self.ctx.enable_ft4_softbits(soft)
        self.ctx.enable_ft4_decode(decode, *RC.DECODE4)
        self.ctx.enable_ft4_osd(osd, *RC.OSD4)

    def push(self, e):
        iq, step = RC4.slot_iq(e), 64 * RC4.BLK
        for k in range(0, len(iq), step):
            self.ctx.push_iq(self.rx, iq[k:k + step])

    def slot(self, e):
        self.push(e)
        self.ctx.slot_boundary(MODE, RC4.start_epoch(e + 1))


def _want(ctx, dec, seed=RC4.SEED):
    """ft4_decode_reports_ref on the GPU's own frame spectra and sync records of the channels that `dec` names."""
    from oracle import oracle as orc
    chans = sorted({int(c) for c in dec["ch_id"]})
    cx = {ch: ctx.sync_debug(ch, "ft4_cx") for ch in chans}
    recs = {ch: ctx.fetch_ft4_sync(ch, 1800) for ch in chans}
    return R4.reports(orc, K.encoder(seed), cx, recs, dec)


def _check(ctx, E=0, seed=RC4.SEED, max_out=BIG):
    """One call against cwslg_fetch_decodes and the restatement; -> (dec, rep, E, n_total, n_channels)."""
    plain = ctx.fetch_decodes(MODE, E, max_out)
    got = ctx.fetch_ft4_decode_reports(E, max_out)
    assert (plain is None) == (got is None)
    if got is None:
        return None
    dec, rep, E_got, n_total, n_ch = got
    assert (E_got, n_total, n_ch) == plain[1:] and dec.dtype == DR.DECODE_DTYPE and dec.tobytes() == plain[0].tobytes()
    assert rep.dtype == R4.REPORT_DTYPE and len(rep) == len(dec)
    want = _want(ctx, dec, seed)
    bad = [p for p in range(len(dec)) if rep[p].tobytes() != want[p].tobytes()]
    assert not bad, (bad[:5], rep[bad[:3]], want[bad[:3]], dec[bad[:3]])
    return got


def _nsync_equals_the_soft_records(ctx, dec, rep):
    for ch in sorted({int(c) for c in dec["ch_id"]}):
        nsync = np.asarray(ctx.fetch_ft4_softbits(ch, 1800)[2])
        sel = dec["ch_id"] == ch
        assert np.array_equal(rep["nsync"][sel], nsync[dec["entry"][sel]])


# ---- the vetted recipe ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_cand", [1, 5, 100])
@pytest.mark.parametrize("osd", [True, False], ids=["osd", "no_osd"])
@pytest.mark.parametrize("n_chan", [1, 2])
def test_reports_against_the_restatement(xctx, n_chan, osd, max_cand):
    g = _Group(xctx, RC4.RF[:n_chan], max_cand, osd=osd)
    assert xctx.fetch_ft4_decode_reports() is None                      # the first boundary discards: nothing yet
    seen_d, seen = np.zeros(0, DR.DECODE_DTYPE), np.zeros(0, R4.REPORT_DTYPE)
    for e in range(RC4.N_EPOCHS):
        g.slot(e)
        dec, rep, E, n_total, n_ch = _check(xctx)
        assert (E, n_ch) == (RC4.start_epoch(e), n_chan) and n_total == len(dec)
        _nsync_equals_the_soft_records(xctx, dec, rep)
        again = xctx.fetch_ft4_decode_reports(E, BIG)                   # two calls on one epoch: the same bytes
        assert again[2:] == (E, n_total, n_ch) and again[0].tobytes() == dec.tobytes() and again[1].tobytes() == rep.tobytes()
        seen_d, seen = np.concatenate([seen_d, dec]), np.concatenate([seen, rep])
    if max_cand == 100 and osd:
        # (the slots do contain what they were made for: test_ft4_decode_reports_inputs.py proves it on the CPU chain): the twin slots' ndup > 1,
        # words OSD alone returns, sets other than 0, nsymerr 0 and above, a report at the floor and reports that are not
        assert (seen["nsymerr"] == 0).any() and (seen["nsymerr"] > 0).any() and (seen["snr_db"] == -21).any() and (seen["snr_db"] > -21).any()
        assert seen_d["ndup"].max() > 1 and seen_d["by_osd"].any() and seen_d["set"].any() and not seen_d["by_osd"].all()


# ---- truncation ---------------------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, E, dec, rep, mx, with_channels=True):
    t0, n, nt, nc = C.c_uint64(E), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = ctx.L.cwslg_fetch_ft4_decode_reports(ctx.h, C.byref(t0), None if dec is None else dec.ctypes.data, None if rep is None else rep.ctypes.data, mx,
                                              C.byref(n), C.byref(nt), C.byref(nc) if with_channels else None)
    return rc, t0.value, n.value, nt.value, nc.value


def test_truncation_by_max(xctx):
    """max = 0, 1, n_total - 1, n_total, n_total + 1; a null dec or a null rep: n = min(n_total, max), the first n of the full answer, and not a byte
    written beyond record n of either block."""
    g = _Group(xctx, RC4.RF, 100)
    g.slot(0)
    full_dec, full_rep, E0, total, _ = _check(xctx)
    assert total >= 3
    for mx in (0, 1, total - 1, total, total + 1):
        for null in ("", "dec", "rep"):
            dec = None if null == "dec" else np.full(total + 2, 0xAB, np.uint8).repeat(40).view(DR.DECODE_DTYPE)
            rep = None if null == "rep" else np.full(total + 2, 0xAB, np.uint8).repeat(16).view(R4.REPORT_DTYPE)
            rc, E, n, nt, nc = _raw(xctx, 0, dec, rep, mx)
            assert (rc, E, n, nt, nc) == (0, E0, min(total, mx), total, 2), (mx, null, rc, E, n, nt, nc)
            if dec is not None:
                assert dec[:n].tobytes() == full_dec[:n].tobytes() and set(dec[n:].tobytes()) == {0xAB}
            if rep is not None:
                assert rep[:n].tobytes() == full_rep[:n].tobytes() and set(rep[n:].tobytes()) == {0xAB}
    assert _raw(xctx, 0, None, None, 5) == (0, E0, min(total, 5), total, 2)
    assert _raw(xctx, 0, None, None, 0, with_channels=False)[:4] == (0, E0, 0, total)


# ---- many channels --------------------------------------------------------------------------------------------------------------------------------------
def _own_bytes(ctx, chans):
    out = []
    for ch in chans:
        lst, soft, msg, osd = (f(ch, 1800, with_epoch=True) for f in (ctx.fetch_ft4_sync, ctx.fetch_ft4_softbits, ctx.fetch_ft4_decode, ctx.fetch_ft4_osd))
        out.append((repr(lst), None if soft is None else tuple(np.asarray(a).tobytes() for a in soft[:-1]) + (soft[-1],),
                    None if msg is None else (msg[0].tobytes(), msg[1]), None if osd is None else (osd[0].tobytes(), osd[1])))
    return out


@pytest.mark.parametrize("n_chan", [3, 37])
def test_many_channels(xctx, n_chan):
    """3 and 37 FT4 channels on one receiver, list limit 12: the channels whose passband holds the transmissions decode them, the others hear
    noise -- runs of channels without decodes, so the offsets search crosses equal offsets.  The per-channel fetches return the same bytes
    before and after the call; stats.sync_launches does not move."""
    lo, hi = -17400, -13000
    rfs = [RC4.RF[0], RC4.RF[1], RC4.RF[0] + 150][:min(n_chan, 3)] + [int(round(lo + (hi - lo) * j / max(n_chan - 4, 1))) for j in range(n_chan - 3)]
    g = _Group(xctx, rfs, 12)
    g.push(1)
    xctx.slot_boundary(MODE, RC4.start_epoch(1))
    before = _own_bytes(xctx, g.chans)
    launches = xctx.stats()["sync_launches"]
    got = xctx.fetch_ft4_decode_reports(0, BIG)
    assert xctx.stats()["sync_launches"] == launches
    assert _own_bytes(xctx, g.chans) == before
    dec, rep, E, n_total, n_ch = _check(xctx)
    assert got[0].tobytes() == dec.tobytes() and got[1].tobytes() == rep.tobytes()
    assert n_ch == n_chan and n_total >= 3 and len(set(dec["ch_id"])) >= 2
    with_decodes = set(int(c) for c in dec["ch_id"])
    assert any(ch not in with_decodes for ch in g.chans)                # channels without decodes: equal offsets
    _nsync_equals_the_soft_records(xctx, dec, rep)
    cut = xctx.fetch_ft4_decode_reports(E, n_total - 1)
    assert cut[2:] == (E, n_total, n_chan) and cut[0].tobytes() == dec[:-1].tobytes() and cut[1].tobytes() == rep[:-1].tobytes()


# ---- epochs ------------------------------------------------------------------------------------------------------------------------------------------------
def test_epochs_and_switches(xctx):
    """Explicit E, 0 = newest, a stale E; after a boundary with the decode off nothing to fetch; after one with OSD off BP words only."""
    g = _Group(xctx, RC4.RF, 100)
    g.slot(0)
    E0, E1, E2 = (RC4.start_epoch(e) for e in range(3))
    for ask in (0, E0):
        assert _check(xctx, ask)[2] == E0
    assert xctx.fetch_ft4_decode_reports(E1, BIG) is None and xctx.fetch_ft4_decode_reports(E0 + 1, BIG) is None
    g.stages(decode=False)
    g.slot(1)
    assert all(xctx.fetch_ft4_decode_reports(ask, BIG) is None for ask in (0, E0, E1))
    g.stages(osd=False)
    g.push(0)
    xctx.slot_boundary(MODE, RC4.start_epoch(3))
    dec, rep, E, n_total, n_ch = _check(xctx)
    assert (E, n_ch) == (E2, 2) and not dec["by_osd"].any() and n_total > 0
    assert xctx.fetch_ft4_decode_reports(E1, BIG) is None


def test_one_channel_advanced_alone(xctx):
    g = _Group(xctx, RC4.RF, 100, fire=False)
    xctx.slot_boundary(MODE, RC4.start_epoch(0))
    g.slot(0)
    late = xctx.channel_open(g.rx, RC4.RF[0] + 100, MODE)
    E0, E1 = RC4.start_epoch(0), RC4.start_epoch(1)
    dec, rep, E, n_total, n_ch = _check(xctx)
    assert (E, n_ch) == (E0, 2) and late not in dec["ch_id"]
    g.push(1)
    xctx.slot_boundary_channel(g.chans[0], RC4.start_epoch(2))
    dec, rep, E, n_total, n_ch = _check(xctx)
    assert (E, n_ch) == (E1, 1) and set(dec["ch_id"]) <= {g.chans[0]}
    got = _check(xctx, E0)
    assert got[2:] == (E0, got[3], 1) and set(got[0]["ch_id"]) <= {g.chans[1]}
    xctx.channel_close(g.chans[0])
    assert _check(xctx)[2:] == (E0, got[3], 1)
    xctx.channel_close(g.chans[1])
    assert xctx.fetch_ft4_decode_reports(0, BIG) is None


def test_second_code_and_a_table_without_systematic_form(xctx):
    """The report uses the code in force at the call: after a second cwslg_set_ldpc_code the same words are re-encoded under the new table; a
    table whose columns 91..173 are singular loads (and decodes) but has no reports -- CWSLG_ERR_ARG with a text, the decodes untouched."""
    g = _Group(xctx, RC4.RF, 100)
    g.slot(0)
    dec, rep, E, n_total, n_ch = _check(xctx)
    assert np.array_equal(xctx.ft4_tones(dec["bits"][0]), R4.tones(K.encoder(RC4.SEED), dec["bits"][0]))
    xctx.set_ldpc_code(LC.make_code(LC.SEEDS[1])["nm"])
    dec2, rep2, E2, n2, _ = _check(xctx, seed=LC.SEEDS[1])
    assert dec2.tobytes() == dec.tobytes() and (E2, n2) == (E, n_total) and rep2.tobytes() != rep.tobytes()
    assert np.array_equal(xctx.ft4_tones(dec["bits"][0]), R4.tones(K.encoder(LC.SEEDS[1]), dec["bits"][0]))
    xctx.set_ldpc_code(K.singular_table(RC4.SEED))                      # accepted: a code, of rank 83, without a systematic form
    d = np.full(n_total, 0xAB, np.uint8).repeat(40).view(DR.DECODE_DTYPE)
    r = np.full(n_total, 0xAB, np.uint8).repeat(16).view(R4.REPORT_DTYPE)
    rc, _, n, nt, nc = _raw(xctx, 0, d, r, n_total)
    assert (rc, n, nt, nc) == (ERR_ARG, 0, 0, 0) and set(d.tobytes()) == {0xAB} and set(r.tobytes()) == {0xAB}
    assert b"singular" in xctx.L.cwslg_last_error(xctx.h)
    tones = np.zeros(103, np.uint8)
    bits = np.ascontiguousarray(dec["bits"][0])
    assert xctx.L.cwslg_ft4_tones(xctx.h, bits.ctypes.data, tones.ctypes.data) == ERR_ARG and not tones.any()
    plain = xctx.fetch_decodes(MODE, 0, BIG)                            # the decodes themselves are untouched
    assert plain[0].tobytes() == dec.tobytes()
    xctx.set_ldpc_code(LC.make_code(RC4.SEED)["nm"])
    again = xctx.fetch_ft4_decode_reports(0, BIG)
    assert again[0].tobytes() == dec.tobytes() and again[1].tobytes() == rep.tobytes()


# ---- error paths ----------------------------------------------------------------------------------------------------------------------------------------
def test_error_paths(xctx):
    import cwsl_digi_amd as P
    L, h = xctx.L, xctx.h
    dec, rep = np.zeros(4, DR.DECODE_DTYPE), np.zeros(4, R4.REPORT_DTYPE)
    t0, n, nt, nc = C.c_uint64(0), C.c_int(7), C.c_int(7), C.c_int(7)
    xctx.set_ldpc_code(LC.make_code(RC4.SEED)["nm"])
    assert L.cwslg_fetch_ft4_decode_reports(None, C.byref(t0), dec.ctypes.data, rep.ctypes.data, 4, C.byref(n), C.byref(nt), C.byref(nc)) == ERR_ARG
    assert L.cwslg_fetch_ft4_decode_reports(h, None, dec.ctypes.data, rep.ctypes.data, 4, C.byref(n), C.byref(nt), C.byref(nc)) == ERR_ARG
    assert L.cwslg_fetch_ft4_decode_reports(h, C.byref(t0), dec.ctypes.data, rep.ctypes.data, 4, None, C.byref(nt), C.byref(nc)) == ERR_ARG
    assert L.cwslg_fetch_ft4_decode_reports(h, C.byref(t0), dec.ctypes.data, rep.ctypes.data, 4, C.byref(n), None, C.byref(nc)) == ERR_ARG
    # the FT8 call keeps refusing the FT4 group
    assert L.cwslg_fetch_decode_reports(h, P.GROUPS["FT4"], C.byref(t0), dec.ctypes.data, rep.ctypes.data, 4, C.byref(n), C.byref(nt), C.byref(nc)) == ERR_ARG
    # an FT8-only context: no FT4 channel takes part
    xctx.enable_sync(True, 1.2, 10, 200, 3000)
    rx = xctx.receiver_open(RC4.FS, RC.BLK["FT8"], 0)
    xctx.channel_open(rx, RC.RF["FT8"][0], "FT8")
    n.value = nt.value = nc.value = 7
    assert L.cwslg_fetch_ft4_decode_reports(h, C.byref(t0), dec.ctypes.data, rep.ctypes.data, 4, C.byref(n), C.byref(nt), C.byref(nc)) == NO_FRAME
    assert (n.value, nt.value, nc.value, t0.value) == (0, 0, 0, 0)
    tones = np.zeros(103, np.uint8)
    bits = np.zeros(12, np.uint8)
    assert L.cwslg_ft4_tones(None, bits.ctypes.data, tones.ctypes.data) == ERR_ARG
    assert L.cwslg_ft4_tones(h, None, tones.ctypes.data) == ERR_ARG and L.cwslg_ft4_tones(h, bits.ctypes.data, None) == ERR_ARG


def test_no_code_loaded():
    import cwsl_digi_amd as P
    c = P.Context(0)
    try:
        dec, rep = np.zeros(1, DR.DECODE_DTYPE), np.zeros(1, R4.REPORT_DTYPE)
        t0, n, nt = C.c_uint64(0), C.c_int(7), C.c_int(7)
        assert c.L.cwslg_fetch_ft4_decode_reports(c.h, C.byref(t0), dec.ctypes.data, rep.ctypes.data, 1, C.byref(n), C.byref(nt), None) == ERR_ARG
        tones, bits = np.zeros(103, np.uint8), np.zeros(12, np.uint8)
        assert c.L.cwslg_ft4_tones(c.h, bits.ctypes.data, tones.ctypes.data) == ERR_ARG
    finally:
        c.close()
