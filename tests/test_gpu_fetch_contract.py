"""GPU: one argument contract for the eight list / record fetches of the sync stage -- cwslg_fetch_candidates, cwslg_fetch_ft8_softbits / _decode /
_osd and cwslg_fetch_ft4_sync / _softbits / _decode / _osd -- called through the C ABI itself (null pointers included).  One context holds an FT8
channel, an FT4 channel and a JT65 channel (a mode without a sync stage), max_cand = 5, every stage on, the slots of tests/record_race_cases.py.
A table says, per fetch, what each situation returns: status, count, whether the epoch is written, and which bytes of the destination change.
Everything is equality; what the records hold is pinned elsewhere (tests/test_gpu_record_fetch_races.py)."""
import collections
import ctypes as C

import pytest

import ldpc_cases as LC
import record_race_cases as RC

pytestmark = pytest.mark.gpu
OK, ERR_MODE, ERR_ARG, NO_FRAME = 0, -5, -6, -9
MAX_CAND = 5
BIG = 1000                                                              # a `max` far above max_cand (and above 3 records per candidate)
N_SENT, T_SENT, FILL = -77, 0xDEADBEEFCAFEF00D, 0xA5                    # what *n, *start_epoch and the destination hold before a call

# fetch -> (mode of its channel, record type of cwsl_digi_amd.api, text of its mode gate or None)
FETCHES = collections.OrderedDict([
    ("fetch_candidates", ("both", "Candidate", None)),
    ("fetch_ft8_softbits", ("FT8", "Ft8Soft", "soft bits exist for FT8 channels only (mode {})")),
    ("fetch_ft8_decode", ("FT8", "Ft8Msg", "decode records exist for FT8 channels only (mode {})")),
    ("fetch_ft8_osd", ("FT8", "OsdMsg", "OSD records exist for FT8 channels only (mode {})")),
    ("fetch_ft4_sync", ("FT4", "Ft4Sync", None)),
    ("fetch_ft4_softbits", ("FT4", "Ft4Soft", "FT4 soft bits exist for FT4 channels only (mode {})")),
    ("fetch_ft4_decode", ("FT4", "Ft4Msg", "FT4 decode records exist for FT4 channels only (mode {})")),
    ("fetch_ft4_osd", ("FT4", "Ft4Osd", "FT4 OSD records exist for FT4 channels only (mode {})")),
])
CHAIN = {"FT8": ("fetch_ft8_softbits", "fetch_ft8_decode", "fetch_ft8_osd"), "FT4": ("fetch_ft4_sync", "fetch_ft4_softbits", "fetch_ft4_decode", "fetch_ft4_osd")}
# The emitting boundaries, in order: (phase, the fetches that have nothing to hand out after it).  Every other fetch answers with the epoch of the
# frame that boundary emitted -- except after "sync off", where the lists of the boundary before survive under THEIR epoch.
PHASES = (("all on", ()),
          ("all on again", ()),
          ("osd off", ("fetch_ft8_osd", "fetch_ft4_osd")),
          ("decode off", ("fetch_ft8_decode", "fetch_ft8_osd", "fetch_ft4_decode", "fetch_ft4_osd")),
          ("soft off", CHAIN["FT8"] + CHAIN["FT4"][1:]),
          ("coherent off", CHAIN["FT4"]),                               # (the FT8 chain, switched on again, answers)
          ("sync off", CHAIN["FT8"] + CHAIN["FT4"]))
Obs = collections.namedtuple("Obs", "rc n t0 buf error")


def _targets(name):
    mode = FETCHES[name][0]
    return ("FT8", "FT4") if mode == "both" else (mode,)


class _Run:
    def __init__(self, ctx):
        from cwsl_digi_amd import api
        self.ctx, self.api = ctx, api
        ctx.enable_sync(True, RC.SYNC["syncmin"], MAX_CAND, RC.SYNC["f_lo"], RC.SYNC["f_hi"])
        ctx.set_ft4_syncmin(RC.SYNCMIN_FT4)
        ctx.set_ldpc_code(LC.make_code(RC.SEED)["nm"])
        self.rx = {m: ctx.receiver_open(RC.FS, RC.BLK[m], 0) for m in RC.MODES}
        self.ch = {m: ctx.channel_open(self.rx[m], RC.RF[m][0], m) for m in RC.MODES}
        self.ch["JT65"] = ctx.channel_open(self.rx["FT8"], RC.RF["FT8"][1], "JT65")
        self.fired = 0
        self.obs = {}                                                   # (situation, fetch, channel key) -> Obs

    def call(self, name, ch, max_, cap=None, dst=True, n=True, epoch=True):
        rec = getattr(self.api, FETCHES[name][1])
        nbytes = max(cap if cap is not None else max_, 1) * C.sizeof(rec)
        buf = (C.c_ubyte * nbytes)()
        C.memset(buf, FILL, nbytes)
        nn, t0 = C.c_int(N_SENT), C.c_uint64(T_SENT)
        rc = getattr(self.ctx.L, "cwslg_" + name)(self.ctx.h, ch, C.cast(buf, C.POINTER(rec)) if dst else None, max_, C.byref(nn) if n else None,
                                                   C.byref(t0) if epoch else None)
        return Obs(rc, nn.value, t0.value, bytes(buf), self.ctx.L.cwslg_last_error(self.ctx.h).decode() if rc not in (OK, NO_FRAME) else "")

    def item(self, name):
        return C.sizeof(getattr(self.api, FETCHES[name][1]))

    def boundary(self):
        """Both groups: a slot of IQ (none before the first boundary, which discards), then the boundary."""
        for m in RC.MODES:
            if self.fired:
                iq, step = RC.slot_iq(m, (self.fired - 1) % 2), 64 * RC.BLK[m]
                for k in range(0, len(iq), step):
                    self.ctx.push_iq(self.rx[m], iq[k:k + step])
            self.ctx.slot_boundary(m, RC.start_epoch(m, self.fired))
        self.fired += 1

    def sweep(self, situation):
        """Every fetch on every channel it is meant for, with room for everything."""
        for name in FETCHES:
            for m in _targets(name):
                self.obs[(situation, name, m)] = self.call(name, self.ch[m], BIG)

    def switches(self, phase):
        c = self.ctx
        if phase == "osd off":
            c.enable_ft8_osd(False); c.enable_ft4_osd(False)
        elif phase == "decode off":
            c.enable_ft8_osd(True, *RC.OSD8); c.enable_ft4_osd(True, *RC.OSD4)
            c.enable_ft8_decode(False); c.enable_ft4_decode(False)
        elif phase == "soft off":
            c.enable_ft8_decode(True, *RC.DECODE8); c.enable_ft4_decode(True, *RC.DECODE4)
            c.enable_ft8_softbits(False); c.enable_ft4_softbits(False)
        elif phase == "coherent off":
            c.enable_ft8_softbits(True); c.enable_ft4_softbits(True)
            c.enable_ft4_coherent(False)
        elif phase == "sync off":
            c.enable_ft4_coherent(True)
            c.enable_sync(False)

    def arguments(self):
        """The argument situations, on the results of the first emitting boundary."""
        for name in FETCHES:
            for m in _targets(name):
                ch, full = self.ch[m], self.obs[("all on", name, m)]
                o = self.obs
                o[("n null", name, m)] = self.call(name, ch, BIG, n=False)
                o[("dst null", name, m)] = self.call(name, ch, 3, dst=False)
                o[("max 0", name, m)] = self.call(name, ch, 0, dst=False)
                o[("max 1", name, m)] = self.call(name, ch, 1, cap=full.n)
                o[("max n-1", name, m)] = self.call(name, ch, full.n - 1, cap=full.n)
                o[("max n", name, m)] = self.call(name, ch, full.n, cap=full.n + 1)
                o[("epoch null", name, m)] = self.call(name, ch, BIG, epoch=False)
            for bad in (-1, 1000):
                self.obs[("bad id", name, bad)] = self.call(name, bad, BIG)
            for m in ("FT8", "FT4", "JT65"):                            # every channel the fetch is not meant for
                if m not in _targets(name):
                    self.obs[("other channel", name, m)] = self.call(name, self.ch[m], BIG)


@pytest.fixture(scope="module")
def run():
    import cwsl_digi_amd as P
    ctx = P.Context(0)
    try:
        r = _Run(ctx)
        ctx.enable_ft8_softbits(True); ctx.enable_ft8_decode(True, *RC.DECODE8); ctx.enable_ft8_osd(True, *RC.OSD8)
        ctx.enable_ft4_softbits(True); ctx.enable_ft4_decode(True, *RC.DECODE4); ctx.enable_ft4_osd(True, *RC.OSD4)
        r.sweep("before any boundary")
        r.boundary()
        r.sweep("after the discarding boundary")
        for phase, _ in PHASES:
            r.switches(phase)
            r.boundary()
            r.sweep(phase)
            if phase == "all on":
                r.arguments()
        yield r
    finally:
        ctx.close()


def _epoch(m, phase_index):
    return RC.start_epoch(m, phase_index)                               # phase k's boundary emits the frame that started at boundary k


@pytest.mark.parametrize("name", list(FETCHES))
def test_nothing_before_the_first_frame(run, name):
    for situation in ("before any boundary", "after the discarding boundary"):
        for m in _targets(name):
            o = run.obs[(situation, name, m)]
            assert (o.rc, o.n, o.t0) == (NO_FRAME, 0, T_SENT) and set(o.buf) == {FILL}, (situation, m, o[:3])


@pytest.mark.parametrize("name", list(FETCHES))
def test_full_fetch_and_its_truncations(run, name):
    item = run.item(name)
    for m in _targets(name):
        full = run.obs[("all on", name, m)]
        assert (full.rc, full.t0) == (OK, _epoch(m, 0)), (m, full[:3])
        ncand = run.obs[("all on", "fetch_candidates", m)].n
        assert ncand == MAX_CAND                                         # the lists are cut: more than max_cand candidates pass
        if name in CHAIN["FT4"]:
            nsync = run.obs[("all on", "fetch_ft4_sync", m)]
            cands = [int.from_bytes(nsync.buf[q * 32 + 28:q * 32 + 32], "little") for q in range(nsync.n)]
            assert full.n == nsync.n > len(set(cands)) >= 2              # a candidate with more than one record
        else:
            assert full.n == ncand
        assert set(full.buf[full.n * item:]) == {FILL} and set(full.buf[:full.n * item]) != {FILL}
        data = full.buf[:full.n * item]
        for situation, k in (("max 1", 1), ("max n-1", full.n - 1), ("max n", full.n)):
            o = run.obs[(situation, name, m)]
            assert (o.rc, o.n, o.t0) == (OK, k, full.t0), (situation, m, o[:3])
            assert o.buf[:k * item] == data[:k * item] and set(o.buf[k * item:]) == {FILL}, (situation, m)      # the first k, and not a byte behind them
        o = run.obs[("epoch null", name, m)]
        assert (o.rc, o.n, o.t0, o.buf) == (OK, full.n, T_SENT, full.buf), (m, o[:3])
        o = run.obs[("max 0", name, m)]
        assert (o.rc, o.n, o.t0) == (OK, 0, full.t0), (m, o[:3])
        again = run.obs[("all on again", name, m)]
        assert (again.rc, again.t0) == (OK, _epoch(m, 1)) and again.n >= 2 and again.buf != full.buf, (m, again[:3])      # the next slot's, not these


@pytest.mark.parametrize("name", list(FETCHES))
def test_bad_arguments(run, name):
    for m in _targets(name):
        o = run.obs[("n null", name, m)]
        assert (o.rc, o.t0) == (ERR_ARG, T_SENT) and set(o.buf) == {FILL}, (m, o[:3])
        o = run.obs[("dst null", name, m)]
        assert (o.rc, o.n, o.t0) == (ERR_ARG, N_SENT, T_SENT), (m, o[:3])
    for bad in (-1, 1000):
        o = run.obs[("bad id", name, bad)]
        assert (o.rc, o.n, o.t0, o.error) == (ERR_ARG, 0, T_SENT, "bad channel id") and set(o.buf) == {FILL}, (bad, o[:3], o.error)


@pytest.mark.parametrize("name", list(FETCHES))
def test_channels_of_another_mode(run, name):
    gate = FETCHES[name][2]
    for m in ("FT8", "FT4", "JT65"):
        if m in _targets(name):
            continue
        o = run.obs[("other channel", name, m)]
        if gate:
            assert (o.rc, o.n, o.t0, o.error) == (ERR_MODE, 0, T_SENT, gate.format(m)), (m, o[:3], o.error)
        else:                                                            # no mode gate: such a channel simply never has these records
            assert (o.rc, o.n, o.t0) == (NO_FRAME, 0, T_SENT), (m, o[:3])
        assert set(o.buf) == {FILL}


@pytest.mark.parametrize("name", list(FETCHES))
def test_a_stage_switched_off_hands_out_nothing(run, name):
    for k, (phase, nothing) in enumerate(PHASES):
        for m in _targets(name):
            o = run.obs[(phase, name, m)]
            if name in nothing:
                assert (o.rc, o.n, o.t0) == (NO_FRAME, 0, T_SENT) and set(o.buf) == {FILL}, (phase, m, o[:3])
            elif phase == "sync off":                                   # the list of the boundary before, under its own epoch
                before = run.obs[(PHASES[k - 1][0], name, m)]
                assert (o.rc, o.n, o.t0, o.buf) == (OK, before.n, _epoch(m, k - 1), before.buf), (phase, m, o[:3])
            else:
                assert (o.rc, o.t0) == (OK, _epoch(m, k)) and o.n >= 2, (phase, m, o[:3])
