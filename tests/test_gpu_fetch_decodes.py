"""GPU: cwslg_fetch_decodes -- the decoded words of a whole FT8 / FT4 slot-clock group in one fetch, chosen and de-duplicated on the device
(include/cwsl_gpu.h, "The decodes of a slot"; csrc/harvest_kernels.hpp).  Every comparison is byte for byte: against tests/decodes_ref.py on the
CPU chain's records (tests/harvest_cases.py), and against decodes_ref on the GPU's own per-channel fetches, which must come back unchanged
after the call."""
import ctypes as C
import threading
import time

import numpy as np
import pytest

import decodes_ref as DR
import harvest_cases as H
import harvest_twin_cases as T
import ldpc_cases as LC
import record_race_cases as RC

pytestmark = pytest.mark.gpu
NO_FRAME, ERR_ARG = -9, -6
BIG = 1 << 16                                                           # a `max` above every total here


@pytest.fixture
def xctx():
    """A fresh context in the default (exact) arithmetic mode: the CPU chain's frames are the oracle's, bit for bit."""
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


def _sync(ctx, mode, max_cand, syncmin=None):
    s = H.SYNC8 if mode == "FT8" else RC.SYNC
    ctx.enable_sync(True, s["syncmin"] if syncmin is None else syncmin, max_cand, s["f_lo"], s["f_hi"])
    ctx.set_ft4_syncmin(RC.SYNCMIN_FT4)


def _stages(ctx, mode, soft=True, decode=True, osd=True):
    if mode == "FT8":
        ctx.enable_ft8_softbits(soft)
        ctx.enable_ft8_decode(decode, *RC.DECODE8)
        ctx.enable_ft8_osd(osd, *RC.OSD8)
    else:
        ctx.enable_ft4_softbits(soft)
        ctx.enable_ft4_decode(decode, *RC.DECODE4)
        ctx.enable_ft4_osd(osd, *RC.OSD4)


class _Group:
    """One mode's receiver and channels, everything on, the first (discarding) boundary fired."""

    def __init__(self, ctx, mode, rfs, max_cand, osd=True, syncmin=None, fire=True):
        self.ctx, self.mode = ctx, mode
        _sync(ctx, mode, max_cand, syncmin)
        ctx.set_ldpc_code(LC.make_code(H.SEED)["nm"])
        _stages(ctx, mode, osd=osd)
        self.rx = ctx.receiver_open(H.FS, H.BLK[mode], 0)
        self.chans = [ctx.channel_open(self.rx, rf, mode) for rf in rfs]
        if fire:
            ctx.slot_boundary(mode, H.start_epoch(mode, 0))

    def push(self, e):
        iq, step = H.slot_iq(self.mode, e), 64 * H.BLK[self.mode]
        for k in range(0, len(iq), step):
            self.ctx.push_iq(self.rx, iq[k:k + step])

    def slot(self, e):
        """Slot e: its IQ and the boundary that ends it."""
        self.push(e)
        self.ctx.slot_boundary(self.mode, H.start_epoch(self.mode, e + 1))


def _own_records(ctx, mode, ch):
    """The GPU's own per-channel fetches of one channel: (list / sync records, decode records, OSD records or None), each with its epoch."""
    if mode == "FT8":
        try:
            lst = ctx.fetch_candidates(ch, 600, with_epoch=True)
        except Exception:
            lst = None
        return lst, ctx.fetch_ft8_decode(ch, 600, with_epoch=True), ctx.fetch_ft8_osd(ch, 600, with_epoch=True)
    return ctx.fetch_ft4_sync(ch, 1800, with_epoch=True), ctx.fetch_ft4_decode(ch, 1800, with_epoch=True), ctx.fetch_ft4_osd(ch, 1800, with_epoch=True)


def _own_bytes(ctx, mode, chans):
    """Everything the per-channel fetches hand out, as bytes: list, soft, decode and OSD records of every channel."""
    out = []
    for ch in chans:
        lst, msg, osd = _own_records(ctx, mode, ch)
        soft = ctx.fetch_ft8_softbits(ch, 600, with_epoch=True) if mode == "FT8" else ctx.fetch_ft4_softbits(ch, 1800, with_epoch=True)
        out.append((repr(lst), None if soft is None else tuple(np.asarray(a).tobytes() for a in soft[:-1]) + (soft[-1],),
                    None if msg is None else (msg[0].tobytes(), msg[1]), None if osd is None else (osd[0].tobytes(), osd[1])))
    return out


def _own_expected(ctx, mode, chans, E, max_out=None):
    """decodes_ref on the GPU's own records of the channels whose decode records are of epoch E."""
    inp = []
    for ch in chans:
        lst, msg, osd = _own_records(ctx, mode, ch)
        if msg is None or msg[1] != E:
            continue
        assert lst is not None and lst[1] == E
        where = DR.where_ft8(lst[0]) if mode == "FT8" else DR.where_ft4(lst[0])
        inp.append((ch, where, msg[0], osd[0] if osd is not None and osd[1] == E else None))
    return DR.decodes(mode, inp, max_out) + (len(inp),)


def _same(got, want):
    assert got.dtype == DR.DECODE_DTYPE and got.tobytes() == want.tobytes(), (len(got), len(want), got[:4], want[:4])


# ---- against the CPU chain -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_cand", [1, 5, 100])
@pytest.mark.parametrize("osd", [True, False], ids=["osd", "no_osd"])
@pytest.mark.parametrize("n_chan", [1, 2])
@pytest.mark.parametrize("mode", H.MODES)
def test_against_the_cpu_chain(xctx, mode, n_chan, osd, max_cand):
    """The three slots of harvest_cases, one boundary each: the call equals decodes_ref on the CPU chain's records of that slot -- records, order,
    n_total, n_channels and the epoch -- with OSD on or off at the boundary and the list cut at 1, 5 or 100."""
    g = _Group(xctx, mode, H.RF[mode][:n_chan], max_cand, osd=osd)
    assert xctx.fetch_decodes(mode) is None                             # the first boundary discards: nothing yet
    for e in range(H.N_EPOCHS):
        g.slot(e)
        want, total = H.expected(mode, g.chans, e, max_cand, osd=osd)
        got, E, n_total, n_ch = xctx.fetch_decodes(mode, 0, BIG)
        assert (E, n_total, n_ch) == (H.start_epoch(mode, e), total, n_chan), (e, E, n_total, n_ch, total)
        _same(got, want)
        again = xctx.fetch_decodes(mode, E, BIG)                        # two calls on one epoch: the same bytes
        assert again[1:] == (E, n_total, n_ch) and again[0].tobytes() == got.tobytes()
    if max_cand == 100 and n_chan == 2 and osd:
        assert total > 0 and (mode == "FT4" or got["ndup"].max() > 1)    # (the slots do contain what they were made for: test_harvest_inputs.py)


@pytest.mark.parametrize("osd", [True, False], ids=["osd", "no_osd"])
def test_ft4_twins_against_the_cpu_chain(xctx, osd):
    """FT4 de-duplication and its rank decisions on real slots: harvest_twin_cases sends one message at two or three audio frequencies of a
    channel, so that one word sits on two BP records with unequal nharderr, on an OSD record with a smaller entry than the BP record that is
    reported, on two OSD records, and on three records (tests/test_harvest_twin_inputs.py proves it).  The call equals decodes_ref on the CPU
    chain's records, with OSD on and off, and the per-channel fetches return the same bytes before and after it."""
    mode = "FT4"
    g = _Group(xctx, mode, T.RF, T.MAX_CAND, osd=osd)
    ndup = 0
    for e in range(T.N_EPOCHS):
        iq, step = T.slot_iq(e), 64 * T.BLK
        for k in range(0, len(iq), step):
            xctx.push_iq(g.rx, iq[k:k + step])
        xctx.slot_boundary(mode, T.start_epoch(e + 1))
        before = _own_bytes(xctx, mode, g.chans)
        want, total = T.expected(g.chans, e, osd=osd)
        got, E, n_total, n_ch = xctx.fetch_decodes(mode, 0, BIG)
        assert (E, n_total, n_ch) == (T.start_epoch(e), total, 2), (e, E, n_total, n_ch, total)
        _same(got, want)
        assert _own_bytes(xctx, mode, g.chans) == before
        ndup = max(ndup, int(got["ndup"].max()))
    assert ndup >= 3


# ---- truncation ------------------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, group, E, dst, mx, with_channels=True):
    t0, n, nt, nc = C.c_uint64(E), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = ctx.L.cwslg_fetch_decodes(ctx.h, group, C.byref(t0), None if dst is None else dst.ctypes.data, mx, C.byref(n), C.byref(nt),
                                   C.byref(nc) if with_channels else None)
    return rc, t0.value, n.value, nt.value, nc.value


@pytest.mark.parametrize("mode", H.MODES)
def test_truncation_by_max(xctx, mode):
    """max = 0, 1, n_total - 1, n_total, n_total + 1, and dst null with max 0: n = min(n_total, max), the first n records of the full answer,
    n_total whole, and not a byte written beyond record n."""
    import cwsl_digi_amd as P
    g = _Group(xctx, mode, H.RF[mode], 100)
    g.slot(0)
    full, total = H.expected(mode, g.chans, 0, 100)
    assert total >= 3
    grp = P.GROUPS[mode]
    for mx in (0, 1, total - 1, total, total + 1):
        dst = np.full(total + 2, 0xAB, np.uint8).repeat(40).view(DR.DECODE_DTYPE)
        rc, E, n, nt, nc = _raw(xctx, grp, 0, dst, mx)
        assert (rc, E, n, nt, nc) == (0, H.start_epoch(mode, 0), min(total, mx), total, 2), (mx, rc, E, n, nt, nc)
        assert dst[:n].tobytes() == full[:n].tobytes()
        assert set(dst[n:].tobytes()) == {0xAB}
    assert _raw(xctx, grp, 0, None, 0) == (0, H.start_epoch(mode, 0), 0, total, 2)
    assert _raw(xctx, grp, 0, None, 0, with_channels=False)[:4] == (0, H.start_epoch(mode, 0), 0, total)


# ---- against the GPU's own records: many channels -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_chan", [3, 5, 257])
def test_many_channels_against_own_records(xctx, n_chan):
    """3, 5 and 257 FT8 channels on one receiver (257: the first count beyond one workgroup's width in the scan), list limit 8, syncmin 2.0: the
    channels whose passband holds harvest_cases' transmissions decode them, the others hear noise and most have an empty list.  The call equals
    decodes_ref on the GPU's own per-channel fetches; those fetches return the same bytes before and after it; stats.sync_launches does not
    move."""
    mode = "FT8"
    lo, hi = -17400, -13000                                             # dial offsets around the transmissions' (-15000 + 500 .. 2750 Hz audio)
    rfs = [H.RF[mode][0], H.RF[mode][1], 6000][:min(n_chan, 3)] + [int(round(lo + (hi - lo) * j / max(n_chan - 4, 1))) for j in range(n_chan - 3)]
    g = _Group(xctx, mode, rfs, 8, syncmin=2.0)
    g.push(1)                                                           # (slot 1's IQ as the context's first slot)
    xctx.slot_boundary(mode, H.start_epoch(mode, 1))
    E = H.start_epoch(mode, 0)
    before = _own_bytes(xctx, mode, g.chans)
    launches = xctx.stats()["sync_launches"]
    got, E_got, n_total, n_ch = xctx.fetch_decodes(mode, 0, BIG)
    assert xctx.stats()["sync_launches"] == launches
    want, total, took_part = _own_expected(xctx, mode, g.chans, E)
    assert (E_got, n_total, n_ch) == (E, total, took_part) and took_part == n_chan
    _same(got, want)
    assert _own_bytes(xctx, mode, g.chans) == before
    lists = [len(xctx.fetch_candidates(ch, 600)) for ch in g.chans]
    assert total >= 3 and list(got["ch_id"]) == sorted(got["ch_id"]) and len(set(got["ch_id"])) >= (1 if n_chan == 3 else 2)
    assert min(lists) == 0 and max(lists) > 0, lists                    # one list at least is empty
    cut = xctx.fetch_decodes(mode, E, total - 1)
    assert cut[1:] == (E, total, n_chan) and cut[0].tobytes() == want[:total - 1].tobytes()


@pytest.mark.parametrize("n_chan", [3, 5])
def test_ft4_channels_against_own_records(xctx, n_chan):
    """The same for FT4 (the nrec walk): record_race_cases' two dial offsets and others beside them, list limit 12."""
    mode = "FT4"
    rfs = list(H.RF[mode]) + [H.RF[mode][0] + 150 * (j + 1) for j in range(n_chan - 2)]
    g = _Group(xctx, mode, rfs, RC.MAX_CAND)
    g.slot(0)
    E = H.start_epoch(mode, 0)
    before = _own_bytes(xctx, mode, g.chans)
    launches = xctx.stats()["sync_launches"]
    got, E_got, n_total, n_ch = xctx.fetch_decodes(mode, 0, BIG)
    assert xctx.stats()["sync_launches"] == launches
    want, total, took_part = _own_expected(xctx, mode, g.chans, E)
    assert (E_got, n_total, n_ch) == (E, total, n_chan) and took_part == n_chan and total >= 5
    _same(got, want)
    assert _own_bytes(xctx, mode, g.chans) == before


# ---- epochs ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", H.MODES)
def test_epochs_and_switches(xctx, mode):
    """Explicit E, 0 = newest, a stale E; after a boundary with the decode off nothing to fetch; after one with OSD off BP words only."""
    mc = RC.MAX_CAND
    g = _Group(xctx, mode, H.RF[mode], mc)
    g.slot(0)
    E0, E1, E2 = (H.start_epoch(mode, e) for e in range(3))
    want0, total0 = H.expected(mode, g.chans, 0, mc)
    for ask in (0, E0):
        got, E, n_total, n_ch = xctx.fetch_decodes(mode, ask, BIG)
        assert (E, n_total, n_ch) == (E0, total0, 2)
        _same(got, want0)
    assert xctx.fetch_decodes(mode, E1, BIG) is None and xctx.fetch_decodes(mode, E0 + 1, BIG) is None
    _stages(xctx, mode, decode=False)                                   # decode off at the boundary that ends slot 1
    g.slot(1)
    assert all(xctx.fetch_decodes(mode, ask, BIG) is None for ask in (0, E0, E1))
    _stages(xctx, mode, osd=False)                                      # decode on again, OSD off
    g.slot(2)
    want2, total2 = H.expected(mode, g.chans, 2, mc, osd=False)
    got, E, n_total, n_ch = xctx.fetch_decodes(mode, 0, BIG)
    assert (E, n_total, n_ch) == (E2, total2, 2) and not got["by_osd"].any()
    _same(got, want2)
    assert xctx.fetch_decodes(mode, E1, BIG) is None                    # stale


def test_one_channel_advanced_alone(xctx):
    """cwslg_slot_boundary_channel moves one channel to the next epoch: 0 returns that channel only, the older epoch the other; a channel opened
    after the boundary, a closed channel and a JS8 channel of the group are not counted."""
    mode, mc = "FT8", 100
    g = _Group(xctx, mode, H.RF[mode], mc, fire=False)
    js8 = xctx.channel_open(g.rx, H.RF[mode][0], "JS8")
    xctx.slot_boundary(mode, H.start_epoch(mode, 0))
    g.slot(0)
    late = xctx.channel_open(g.rx, H.RF[mode][0] + 100, mode)           # opened after the boundary: no frame, no records
    E0, E1 = H.start_epoch(mode, 0), H.start_epoch(mode, 1)
    want, total = H.expected(mode, g.chans, 0, mc)
    got, E, n_total, n_ch = xctx.fetch_decodes(mode, 0, BIG)
    assert (E, n_total, n_ch) == (E0, total, 2) and js8 not in got["ch_id"] and late not in got["ch_id"]
    _same(got, want)
    g.push(1)
    xctx.slot_boundary_channel(g.chans[0], H.start_epoch(mode, 2))      # channel 0 alone ends slot 1
    want1, total1 = H.expected(mode, g.chans, 1, mc, only=[0])
    got, E, n_total, n_ch = xctx.fetch_decodes(mode, 0, BIG)
    assert (E, n_total, n_ch) == (E1, total1, 1)
    _same(got, want1)
    want0, total0 = H.expected(mode, g.chans, 0, mc, only=[1])          # the other channel still holds slot 0
    got, E, n_total, n_ch = xctx.fetch_decodes(mode, E0, BIG)
    assert (E, n_total, n_ch) == (E0, total0, 1)
    _same(got, want0)
    xctx.channel_close(g.chans[0])
    got, E, n_total, n_ch = xctx.fetch_decodes(mode, 0, BIG)
    assert (E, n_total, n_ch) == (E0, total0, 1)
    _same(got, want0)
    xctx.channel_close(g.chans[1])
    assert xctx.fetch_decodes(mode, 0, BIG) is None


def test_second_code_between_boundaries(xctx):
    """A second cwslg_set_ldpc_code between boundaries drains the streams and leaves the records alone: the call returns the same bytes before
    and after it, and the next slot decodes under the code loaded again."""
    mode, mc = "FT8", 100
    g = _Group(xctx, mode, H.RF[mode], mc)
    g.slot(0)
    first = xctx.fetch_decodes(mode, 0, BIG)
    xctx.set_ldpc_code(LC.make_code(LC.SEEDS[1])["nm"])
    again = xctx.fetch_decodes(mode, 0, BIG)
    assert again[1:] == first[1:] and again[0].tobytes() == first[0].tobytes()
    xctx.set_ldpc_code(LC.make_code(H.SEED)["nm"])
    _stages(xctx, mode)                                                 # (loading a code may switch OSD off; everything on again)
    g.slot(1)
    want, total = H.expected(mode, g.chans, 1, mc)
    got, E, n_total, n_ch = xctx.fetch_decodes(mode, 0, BIG)
    assert (E, n_total, n_ch) == (H.start_epoch(mode, 1), total, 2)
    _same(got, want)


# ---- error paths ---------------------------------------------------------------------------------------------------------------------------------------
def test_error_paths(xctx):
    import cwsl_digi_amd as P
    L, h = xctx.L, xctx.h
    dst = np.zeros(4, DR.DECODE_DTYPE)
    t0, n, nt, nc = C.c_uint64(0), C.c_int(7), C.c_int(7), C.c_int(7)
    args = lambda: (C.byref(t0), dst.ctypes.data, 4, C.byref(n), C.byref(nt), C.byref(nc))
    for group in (-1, P.GROUPS["Q65_30"], P.GROUPS["S120"], 8):
        assert L.cwslg_fetch_decodes(h, group, *args()) == ERR_ARG
    assert L.cwslg_fetch_decodes(None, 0, *args()) == ERR_ARG
    assert L.cwslg_fetch_decodes(h, 0, None, dst.ctypes.data, 4, C.byref(n), C.byref(nt), C.byref(nc)) == ERR_ARG
    assert L.cwslg_fetch_decodes(h, 0, C.byref(t0), dst.ctypes.data, 4, None, C.byref(nt), C.byref(nc)) == ERR_ARG
    assert L.cwslg_fetch_decodes(h, 0, C.byref(t0), dst.ctypes.data, 4, C.byref(n), None, C.byref(nc)) == ERR_ARG
    assert L.cwslg_fetch_decodes(h, 0, C.byref(t0), None, 4, C.byref(n), C.byref(nt), C.byref(nc)) == ERR_ARG
    n.value = nt.value = nc.value = 7
    assert L.cwslg_fetch_decodes(h, 0, *args()) == NO_FRAME and (n.value, nt.value, nc.value, t0.value) == (0, 0, 0, 0)      # no channel at all
    assert L.cwslg_fetch_decodes(h, 1, C.byref(t0), None, 0, C.byref(n), C.byref(nt), None) == NO_FRAME


# ---- race -----------------------------------------------------------------------------------------------------------------------------------------------
PAUSE = 0.25                                                            # between two boundaries, as in test_gpu_record_fetch_races.py
JOIN_S = 120.0                                                          # a safeguard, not a measurement


@pytest.mark.parametrize("mode", RC.MODES)
def test_consumer_races_a_free_running_clock(xctx, mode):
    """One consumer calls with *start_epoch = 0 while a clock walks record_race_cases.SCHEDULE over its slots.  Every successful return equals
    decodes_ref on record_race_cases.chain of the epoch it names, under the configuration in force at that boundary; nothing to fetch is
    accepted only while the newest boundary ran without the decode (FT4: or without the coherent stage)."""
    ctx, n_ep = xctx, RC.N_EPOCHS[mode]
    sched = RC.SCHEDULE[mode]
    runs = lambda cfg: cfg.soft and cfg.decode and (mode == "FT8" or cfg.coherent)
    want = {}
    ctx.enable_sync(True, RC.SYNC["syncmin"], RC.MAX_CAND, RC.SYNC["f_lo"], RC.SYNC["f_hi"])
    ctx.set_ldpc_code(LC.make_code(RC.SEED)["nm"])
    rx = ctx.receiver_open(RC.FS, RC.BLK[mode], 0)
    chans = [ctx.channel_open(rx, rf, mode) for rf in RC.RF[mode]]
    for e, cfg in enumerate(sched):
        if runs(cfg):
            inp = []
            for k, ch in enumerate(chans):
                c = RC.chain(mode, k, e, cfg.max_cand)
                inp.append((ch, DR.where_ft8(c["list"]) if mode == "FT8" else DR.where_ft4(c["sync"]), c["msg"], c["osd"] if cfg.osd else None))
            want[RC.start_epoch(mode, e)] = DR.decodes(mode, inp)
    failures, seen, newest, stop = [], set(), [None], threading.Event()

    def configure(cfg):
        ctx.enable_sync(True, RC.SYNC["syncmin"], cfg.max_cand, RC.SYNC["f_lo"], RC.SYNC["f_hi"])
        ctx.set_ft4_syncmin(RC.SYNCMIN_FT4)
        if mode == "FT4":
            ctx.enable_ft4_coherent(cfg.coherent)
        _stages(ctx, mode, soft=cfg.soft, decode=cfg.decode, osd=cfg.osd)

    def clock():
        try:
            configure(sched[0])
            ctx.slot_boundary(mode, RC.start_epoch(mode, 0))
            for e in range(n_ep):
                iq, step = RC.slot_iq(mode, e), 64 * RC.BLK[mode]
                for k in range(0, len(iq), step):
                    ctx.push_iq(rx, iq[k:k + step])
                configure(sched[e])
                ctx.slot_boundary(mode, RC.start_epoch(mode, e + 1))
                newest[0] = e
                time.sleep(PAUSE)
        except Exception as ex:       # pragma: no cover
            failures.append(f"clock: {ex!r}")
        finally:
            stop.set()

    def consumer():
        try:
            while True:
                finished = stop.is_set()
                e_before = newest[0]
                r = ctx.fetch_decodes(mode, 0, BIG)
                e_after = newest[0]
                if r is None:
                    # nothing to fetch: only while the newest boundary (before or after the call, whichever the call met) ran without the decode
                    ok = [e is None or not runs(sched[e]) for e in (e_before, e_after)]
                    if not any(ok):
                        failures.append(f"nothing to fetch although the boundaries of epochs {e_before} / {e_after} ran the decode")
                        return
                else:
                    got, E, n_total, n_ch = r
                    if E not in want:
                        failures.append(f"epoch {E}: no boundary of this run made decode records under it")
                        return
                    w, total = want[E]
                    if (n_total, n_ch) != (total, len(chans)) or got.tobytes() != w.tobytes():
                        failures.append(f"epoch {E}: {n_total} decodes of {n_ch} channels, expected {total} of {len(chans)}; first records {got[:2]} / {w[:2]}")
                        return
                    seen.add(E)
                if finished:
                    return
        except Exception as ex:       # pragma: no cover
            failures.append(f"consumer: {ex!r}")

    threads = [threading.Thread(target=clock, name="clock", daemon=True), threading.Thread(target=consumer, name="consumer", daemon=True)]
    for t in threads:
        t.start()
    deadline = time.monotonic() + JOIN_S
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    if any(t.is_alive() for t in threads):
        ctx.h = None
        pytest.fail("threads still running: a ticket that is never released, or a boundary that waits for ever")
    assert not failures, failures[:3]
    assert len(seen) >= 3 and RC.start_epoch(mode, n_ep - 1) in seen, sorted(seen)
