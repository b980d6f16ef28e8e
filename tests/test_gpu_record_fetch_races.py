"""GPU: the record fetches of the decode chain raced against the next boundary (ABI 5: "results are handed out whole, per epoch").  The seven
fetches behind the candidate lists -- cwslg_fetch_ft8_softbits / _decode / _osd and cwslg_fetch_ft4_sync / _softbits / _decode / _osd -- each
have a stamp of their own and share the ticket, event and epoch logic (csrc/record_kinds.hpp, sync_host.inc); the arithmetic of every stage is pinned elsewhere.  Here a slot
clock runs free while consumers fetch, and ONE rule is applied to whatever comes back: records returned with start epoch e are, byte for byte
(the count included), tests/record_race_cases.py:expected() of that channel, that epoch and the configuration in force at that epoch's
boundary -- and a stage that did not run at e hands out nothing stamped e.  A fetch may come back empty-handed (CWSLG_ERR_NO_FRAME); where that
is an error is said per test.  Every expected value is computed on the CPU before a thread starts (tests/test_record_race_inputs.py vets that
any two epochs differ in every stage), the contexts run in exact mode (the expected frames are the oracle's, bit for bit), and no comparison is
retried: the first mismatch of a consumer is reported with channel, stage, stamped epoch and the first differing record."""
import collections
import threading
import time

import pytest

import ldpc_cases as C
import record_race_cases as RC

pytestmark = pytest.mark.gpu
NO_FRAME = -9                                                           # CWSLG_ERR_NO_FRAME
MAX = 64                                                                # every fetch's `max`: above 3 records for each of MAX_CAND candidates
PAUSE = 0.25                                                            # between two boundaries of a clock: lets the consumers' rounds meet every generation
JOIN_S = 120.0                                                          # a safeguard against a ticket that is never released, not a measurement: the threaded runs take 1.3 to 1.8 s
RECORD_FETCHES = {"FT8": ("fetch_ft8_softbits", "fetch_ft8_decode", "fetch_ft8_osd"),
                  "FT4": ("fetch_ft4_sync", "fetch_ft4_softbits", "fetch_ft4_decode", "fetch_ft4_osd")}


@pytest.fixture
def xctx():
    """A fresh context in the default (exact) arithmetic mode."""
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


# ---- driving the library ------------------------------------------------------------------------------------------------------------------------
def _push(ctx, rx, mode, e):
    iq, step = RC.slot_iq(mode, e), 64 * RC.BLK[mode]
    for k in range(0, len(iq), step):
        ctx.push_iq(rx, iq[k:k + step])


class _Group:
    """One mode's receiver and channels in a context, and the configuration last applied for it."""

    def __init__(self, ctx, mode):
        self.ctx, self.mode = ctx, mode
        self.rx = ctx.receiver_open(RC.FS, RC.BLK[mode], 0)
        self.chans = [ctx.channel_open(self.rx, rf, mode) for rf in RC.RF[mode]]
        self.applied = RC.Config(None, False, False, False, True)     # a new context: nothing enabled, the coherent stage on by default
        self.fired = 0

    def configure(self, cfg):
        """Put cfg in force for this group's next boundary.  The list limit belongs to the context, not to the group, so cwslg_enable_sync is
        called every time (it starts from the default FT4 threshold); a stage is switched only when it changes, so every enable_sync in between
        has to carry the flags over -- which every later epoch's records check."""
        ctx, old = self.ctx, self.applied
        ctx.enable_sync(True, RC.SYNC["syncmin"], cfg.max_cand, RC.SYNC["f_lo"], RC.SYNC["f_hi"])
        ctx.set_ft4_syncmin(RC.SYNCMIN_FT4)
        if self.mode == "FT8":
            if cfg.soft != old.soft:
                ctx.enable_ft8_softbits(cfg.soft)
            if cfg.decode != old.decode:
                ctx.enable_ft8_decode(cfg.decode, *RC.DECODE8)
            if cfg.osd != old.osd:
                ctx.enable_ft8_osd(cfg.osd, *RC.OSD8)
        else:
            if cfg.coherent != old.coherent:
                ctx.enable_ft4_coherent(cfg.coherent)
            if cfg.soft != old.soft:
                ctx.enable_ft4_softbits(cfg.soft)
            if cfg.decode != old.decode:
                ctx.enable_ft4_decode(cfg.decode, *RC.DECODE4)
            if cfg.osd != old.osd:
                ctx.enable_ft4_osd(cfg.osd, *RC.OSD4)
        self.applied = cfg

    def boundary(self, e):
        """The boundary that ends epoch e - 1 (e = 0: the first one, which discards) and starts epoch e."""
        self.ctx.slot_boundary(self.mode, RC.start_epoch(self.mode, e))
        self.fired += 1


def _open(ctx, modes):
    ctx.enable_sync(True, RC.SYNC["syncmin"], RC.MAX_CAND, RC.SYNC["f_lo"], RC.SYNC["f_hi"])
    ctx.set_ldpc_code(C.make_code(RC.SEED)["nm"])
    return {m: _Group(ctx, m) for m in modes}


# ---- the fetches: each -> None (CWSLG_ERR_NO_FRAME) or [(stage, start epoch, byte string)] -------------------------------------------------------
# A byte string of None stands for "the frame came without this": cwslg_fetch_slot hands a list or sync records out only if they belong to the
# frame's epoch.
def _fetch(ctx, mode, name, ch):
    if name == "fetch_frame":
        r = ctx.fetch_frame(ch)
        return None if r is None else [("frame", r["t_start"], r["i16"].tobytes())]
    if name == "fetch_slot":
        r = ctx.fetch_slot(ch, max_list=MAX, max_ft4=MAX)
        if r is None:
            return None
        out = [("frame", r["t_start"], r["i16"].tobytes()), ("list", r["t_start"], RC.list_bytes(r["list"]) if r["list_kind"] == mode else None)]
        if mode == "FT4":
            out.append(("sync", r["t_start"], RC.sync_bytes(r["ft4_sync"]) if r["ft4_sync"] else None))
        return out
    if name == "fetch_candidates":
        from cwsl_digi_amd.api import CwslGpuError
        try:
            lst, t = ctx.fetch_candidates(ch, MAX, with_epoch=True)
        except CwslGpuError as ex:
            if ex.status != NO_FRAME:
                raise
            return None
        return [("list", t, RC.list_bytes(lst))]
    r = getattr(ctx, name)(ch, MAX, with_epoch=True)
    if r is None:
        return None
    if name == "fetch_ft4_sync":
        return [("sync", r[1], RC.sync_bytes(r[0]))]
    if name == "fetch_ft8_softbits":
        return [("soft", r[3], RC.soft8_bytes(*r[:3]))]
    if name == "fetch_ft4_softbits":
        return [("soft", r[4], RC.soft4_bytes(*r[:4]))]
    return [("msg" if name.endswith("decode") else "osd", r[1], r[0].tobytes())]


class _Judge:
    """The single rule, applied to what a fetch returned; collects failures (a thread never raises), the epochs seen per mode and stage, and how
    many fetches came back empty-handed."""

    def __init__(self, config_at):
        self.config_at = config_at                                      # (mode, epoch index) -> Config
        self.failures = []
        self.seen = collections.defaultdict(set)                        # (mode, stage) -> epoch indices
        self.nones = collections.Counter()                              # (mode, fetch) -> count
        self.fetches = collections.Counter()
        self.lock = threading.Lock()                                    # (the counters are shared by the consumers)

    def fail(self, text):
        self.failures.append(text)
        return False

    def check(self, mode, k, name, items):
        """-> False after a failure (the consumer stops)."""
        with self.lock:
            self.fetches[(mode, name)] += 1
            self.nones[(mode, name)] += items is None
        if items is None:
            return True
        for stage, t, got in items:
            where = f"{name}, {mode} channel {k}, stage {stage}, stamped start epoch {t}"
            e = RC.epoch_index(mode, t)
            if e is None:
                return self.fail(f"{where}: no epoch of this run")
            cfg = self.config_at(mode, e)
            want = RC.expected(mode, k, e, cfg)[stage]
            if got is None:
                if want is not None:
                    return self.fail(f"{where} (epoch {e}, {cfg}): the frame came without it although the stage ran at that boundary")
            elif want is None:
                return self.fail(f"{where} (epoch {e}, {cfg}): the stage did not run at that boundary, yet {len(got)} bytes came back under its epoch")
            else:
                d = RC.first_difference(mode, stage, got, want)
                if d:
                    return self.fail(f"{where} (epoch {e}, {cfg}): not that epoch's -- {d}")
                if stage not in ("frame",) and len(got) // RC.record_bytes(mode, stage) > (1 if stage == "list" or mode == "FT8" else 3) * cfg.max_cand:
                    return self.fail(f"{where} (epoch {e}, {cfg}): more records than the list limit allows")
                self.seen[(mode, stage)].add(e)
        return True

    def report(self, title, dt):
        seen = {f"{m} {s}": sorted(v) for (m, s), v in sorted(self.seen.items())}
        nones = {f"{m} {n}": f"{self.nones[(m, n)]} of {c}" for (m, n), c in sorted(self.fetches.items())}
        print(f"\n{title}: {dt:.2f} s; epochs seen per stage {seen}; fetches that came back empty-handed {nones}")


def _consumer(ctx, judge, plan, first, stop, none_is_failure):
    """Rounds over `plan`, a list of (mode, channel index, channel id, fetch), starting at entry `first`, until the clocks have finished and
    one more round is done.  none_is_failure: once this consumer has seen results of a channel, a record fetch of that channel may no
    longer come back empty-handed (every stamp is set in the critical section that sets the frame's)."""
    try:
        i, live = first, set()
        while True:
            finished = stop.is_set()
            for _ in range(len(plan)):
                mode, k, ch, name = plan[i % len(plan)]
                i += 1
                items = _fetch(ctx, mode, name, ch)
                if items is None and none_is_failure and (mode, k) in live and name in RECORD_FETCHES[mode]:
                    judge.fail(f"{name}, {mode} channel {k}: nothing to fetch although this consumer had already seen results of the channel")
                    return
                if items is not None:
                    live.add((mode, k))
                if not judge.check(mode, k, name, items):
                    return
            if finished:
                return
    except Exception as ex:           # pragma: no cover
        judge.fail(f"consumer: {ex!r}")


def _run_threads(ctx, threads):
    """Daemon threads joined with a timeout: a thread that is still alive (a ticket never released, a boundary that waits for ever) fails the
    test instead of hanging it -- the context is then abandoned, not destroyed under the thread."""
    for t in threads:
        t.daemon = True
        t.start()
    deadline = time.monotonic() + JOIN_S
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    stuck = [t.name for t in threads if t.is_alive()]
    if stuck:
        ctx.h = None
        pytest.fail(f"threads still running after {JOIN_S:.0f} s: {stuck}")


def _precompute(mode, config_at, n_epochs):
    for k in range(len(RC.RF[mode])):
        for e in range(n_epochs):
            RC.expected(mode, k, e, config_at(mode, e))


def _race_a_free_running_clock(ctx, mode, fetch_names):
    """All stages on throughout; one clock, three consumers."""
    n = RC.N_RACE[mode]
    config_at = lambda m, e: RC.ALL_ON
    _precompute(mode, config_at, n)
    g = _open(ctx, [mode])[mode]
    g.configure(RC.ALL_ON)
    judge, stop = _Judge(config_at), threading.Event()

    def clock():
        try:
            g.boundary(0)
            for e in range(n):
                _push(ctx, g.rx, mode, e)
                g.boundary(e + 1)
                time.sleep(PAUSE)
        except Exception as ex:       # pragma: no cover
            judge.fail(f"clock: {ex!r}")
        finally:
            stop.set()

    plan = [(mode, k, ch, name) for k, ch in enumerate(g.chans) for name in fetch_names]
    t0 = time.monotonic()
    _run_threads(ctx, [threading.Thread(target=clock, name="clock")] +
                 [threading.Thread(target=_consumer, args=(ctx, judge, plan, 2 * j + 1, stop, True), name=f"consumer {j}") for j in range(3)])
    judge.report(f"{mode} record fetches against a free-running clock", time.monotonic() - t0)
    assert not judge.failures, judge.failures[:3]
    assert g.fired == n + 1
    for stage in RC.STAGES[mode]:                                       # the consumers overlapped several generations of every stage
        assert n - 1 in judge.seen[(mode, stage)] and len(judge.seen[(mode, stage)]) >= 3, (stage, sorted(judge.seen[(mode, stage)]))


def test_ft8_record_fetches_race_a_free_running_clock(xctx):
    """Soft bits, decode and OSD (order 2) on throughout.  A clock thread pushes each epoch's slot and fires the FT8 boundary, back to back, while
    three consumers loop over both channels and the five fetches in rotating order.  Whatever comes back is judged against its OWN stamp (records
    of different stages fetched back to back need not be of one epoch); once a consumer has seen results of a channel, a record fetch that comes
    back empty-handed is a failure; every stage must have been seen at three or more epochs, the last included."""
    _race_a_free_running_clock(xctx, "FT8", RECORD_FETCHES["FT8"] + ("fetch_candidates", "fetch_slot"))


def test_ft4_record_fetches_race_a_free_running_clock(xctx):
    """The same for FT4 with the coherent stage, soft bits, decode and OSD on throughout: the four record fetches, the list, and cwslg_fetch_slot,
    whose sync records must be those of the epoch the frame is stamped with."""
    _race_a_free_running_clock(xctx, "FT4", RECORD_FETCHES["FT4"] + ("fetch_candidates", "fetch_slot"))


# ---- toggles and reallocation --------------------------------------------------------------------------------------------------------------------
ELEVEN = [("FT8", n) for n in RECORD_FETCHES["FT8"] + ("fetch_frame", "fetch_candidates", "fetch_slot")] + \
         [("FT4", n) for n in RECORD_FETCHES["FT4"] + ("fetch_slot",)]
SCHEDULED = lambda mode, e: RC.SCHEDULE[mode][e]


def _plan(groups):
    return [(mode, k, ch, name) for mode, name in ELEVEN for k, ch in enumerate(groups[mode].chans)]


def test_toggles_and_reallocation_under_fetch(xctx):
    """One context, FT8 channels on one receiver and FT4 channels on a second, a clock thread per group, three consumers that mix all eleven
    fetches.  Between its boundaries each clock walks record_race_cases.SCHEDULE -- all on, OSD off, decode off, all on again, (FT4: the coherent
    stage off,) the list limit cut to 5, back to 12 -- so that every boundary frees or reallocates record arrays while the other group's readers
    and this group's late readers are at work.  The list limit is the context's, so a clock sets its configuration and fires its boundary under
    a lock shared with the other clock; nothing else is serialised.  The single rule with the schedule's configuration: a stage switched off at
    an epoch never hands out records stamped with it, a cut list brings no more records than the cut allows, no status other than
    CWSLG_ERR_NO_FRAME is seen, both clocks finish (a ticket that is never released would stop one), both groups are seen at three or more
    epochs."""
    ctx = xctx
    for mode in RC.MODES:
        _precompute(mode, SCHEDULED, RC.N_EPOCHS[mode])
    groups = _open(ctx, RC.MODES)
    judge, cfg_lock = _Judge(SCHEDULED), threading.Lock()
    running = {m: threading.Event() for m in RC.MODES}

    def clock(mode):
        g = groups[mode]
        try:
            with cfg_lock:
                g.configure(RC.SCHEDULE[mode][0])
                g.boundary(0)
            for e in range(RC.N_EPOCHS[mode]):
                _push(ctx, g.rx, mode, e)
                with cfg_lock:
                    g.configure(RC.SCHEDULE[mode][e])
                    g.boundary(e + 1)
                time.sleep(PAUSE)
        except Exception as ex:       # pragma: no cover
            judge.fail(f"{mode} clock: {ex!r}")
        finally:
            running[mode].set()

    class _Both:
        is_set = staticmethod(lambda: all(ev.is_set() for ev in running.values()))

    plan = _plan(groups)
    t0 = time.monotonic()
    _run_threads(ctx, [threading.Thread(target=clock, args=(m,), name=f"{m} clock") for m in RC.MODES] +
                 [threading.Thread(target=_consumer, args=(ctx, judge, plan, 7 * j + 1, _Both, False), name=f"consumer {j}") for j in range(3)])
    judge.report("toggles and reallocation under fetch", time.monotonic() - t0)
    assert not judge.failures, judge.failures[:3]
    for mode in RC.MODES:
        assert groups[mode].fired == RC.N_EPOCHS[mode] + 1
        epochs = set().union(*(judge.seen[(mode, s)] for s in RC.STAGES[mode]))
        assert len(epochs) >= 3 and RC.N_EPOCHS[mode] - 1 in epochs, (mode, sorted(epochs))
        assert len(judge.seen[(mode, "osd")]) >= 2, (mode, sorted(judge.seen[(mode, "osd")]))


def test_late_consumer_after_the_last_boundary(xctx):
    """Single-threaded.  The same two schedules, step by step: after every boundary every fetch of every channel of that group returns that
    epoch's expected values, or nothing where the step's configuration switched the stage off -- and when both schedules have ended, a late
    consumer gets the last epoch's values from every fetch of every channel, twice over, byte for byte the same."""
    ctx = xctx
    for mode in RC.MODES:
        _precompute(mode, SCHEDULED, RC.N_EPOCHS[mode])
    groups = _open(ctx, RC.MODES)
    judge = _Judge(SCHEDULED)
    every = {m: RECORD_FETCHES[m] + ("fetch_frame", "fetch_candidates", "fetch_slot") for m in RC.MODES}

    def round_of(mode, e):
        """Every fetch of every channel of the group: what came back, after the rule; a stage is missing exactly where it did not run at e."""
        out = []
        for k, ch in enumerate(groups[mode].chans):
            want = RC.expected(mode, k, e, SCHEDULED(mode, e))
            for name in every[mode]:
                items = _fetch(ctx, mode, name, ch)
                assert judge.check(mode, k, name, items), judge.failures
                if items is None:
                    stage = {"fetch_ft8_softbits": "soft", "fetch_ft4_softbits": "soft", "fetch_ft4_sync": "sync"}.get(name, "msg" if name.endswith("decode") else "osd")
                    assert name in RECORD_FETCHES[mode] and want[stage] is None, (mode, k, name, e)
                else:
                    assert all(RC.epoch_index(mode, t) == e for _, t, _ in items), (mode, k, name, e, items[0][1])
                out.append((mode, k, name, items))
        return out

    t0 = time.monotonic()
    for mode in RC.MODES:
        g = groups[mode]
        g.configure(RC.SCHEDULE[mode][0])
        g.boundary(0)
        assert all(_fetch(ctx, mode, name, ch) is None for ch in g.chans for name in every[mode])     # the first boundary discards: nothing yet
    for e in range(max(RC.N_EPOCHS.values())):
        for mode in RC.MODES:
            if e < RC.N_EPOCHS[mode]:
                g = groups[mode]
                _push(ctx, g.rx, mode, e)
                g.configure(RC.SCHEDULE[mode][e])
                g.boundary(e + 1)
                round_of(mode, e)
    last = {m: RC.N_EPOCHS[m] - 1 for m in RC.MODES}
    first = [round_of(m, last[m]) for m in RC.MODES]
    again = [round_of(m, last[m]) for m in RC.MODES]
    assert first == again
    assert all(items is not None for r in first for *_, items in r)       # the last step has everything on
    judge.report("late consumer after the last boundary", time.monotonic() - t0)
    assert not judge.failures, judge.failures[:3]
