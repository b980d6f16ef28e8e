"""GPU: the GROUP fetches -- cwslg_fetch_decodes, cwslg_fetch_decode_reports (FT8) and cwslg_fetch_ft4_decode_reports -- raced against the next
boundary, against each other and against a reload of the code.  These calls run real device work on a fetch stream with the context mutex
released (decode_harvest_kernel; decode_report_kernel on the channel's symbol-spectra plane and list; ft4_report_kernel on the
channel's frame spectrum and sync records), protected by the group's ticket, HarvestStage::mu and report_mu alone, while the next boundary
overwrites every buffer they read.  The slots, clocks and helpers are those of tests/test_gpu_record_fetch_races.py; the expected values are
tests/record_race_cases.py:group_expected(), computed on the CPU alone before a thread starts (tests/test_record_race_inputs.py vets them: any
two epochs differ in decodes and in reports, no report sits on its floor, every emitting boundary gives decodes of both channels).

ONE rule for whatever a group fetch returns.  A return stamped E names an epoch of this run whose boundary ran the chain; n_channels == 2;
n_total is the expected total; n == min(n_total, max); the decodes and the reports are, byte for byte, the first n of group_expected under the
configuration in force at that epoch's boundary.  Nothing to fetch (CWSLG_ERR_NO_FRAME) is accepted only before the first emitting boundary,
or while the newest boundary the call can have met ran without the chain: the clock marks a boundary before it fires it and again when it has
returned, and the newest boundary is any from the last one marked returned before the call to the last one marked fired after it.  An
explicit E that is no longer the group's epoch is answered with nothing, never with another epoch's bytes.  No comparison is retried; the
first mismatch of a consumer is reported with the call, its max, the stamped epoch and the first differing record.

Measured on an MI355X in three runs (this module alone, after tests/test_gpu_record_fetch_races.py, in the whole GPU suite).  The threaded part as
report() prints it, and in brackets the call phase in the suite run, which holds the CPU's group_expected as well (the chains are in
record_race_cases' cache by then; alone, the first test to need a mode's chains also pays for them, about 1.7 s for FT8 and 5.5 s for FT4):
    free-running clock, FT8       1.27, 1.27, 1.28 s (1.49 s)     epochs seen 0..4 by every form
    free-running clock, FT4       1.52, 1.52, 1.52 s (2.69 s)     epochs seen 0..5 by every form
    both groups, toggles, reload  2.01, 2.01, 2.01 s (2.01 s)     8 reloads; FT8 epochs 0, 1, 3, 4, 5 and FT4 epochs 0, 1, 3, 5, 6 by every form
    late consumer                 0.08, 0.06, 0.07 s (0.76 s)     the same epochs: every step that ran the chain
The yardstick in the same suite run, the threaded tests of tests/test_gpu_record_fetch_races.py: 1.29, 1.52 and 1.79 s threaded, 1.60, 2.72 and
1.79 s call phase; twice the slowest is 3.6 s (5.4 s), so no test is split.  Calls per form (the call with *start_epoch = 0 and the one that
asks again, counted together) and how many of them came back empty-handed -- before the first emitting boundary, after a boundary without
the chain, or asked for an epoch that had just gone:
    free-running, FT8   9147 to 9922 per form in two runs, 8 to 19 of them empty-handed; 6490 with 232 to 235 in the suite run
    free-running, FT4   8823 to 9484 per form, 14 to 23 empty-handed
    toggles, FT8        5583 to 7445 per form, 865 to 1765 empty-handed;   FT4   4801 to 6479 per form, 1788 to 2727 empty-handed
    late consumer       FT8 8 of 64 per form, FT4 16 of 72: the steps without the chain, and nothing else
"""
import collections
import ctypes as C
import itertools
import threading
import time

import numpy as np
import pytest

import decode_reports_ref as RR
import decodes_ref as DR
import ldpc_cases as LC
import record_race_cases as RC
import test_gpu_record_fetch_races as RF

pytestmark = pytest.mark.gpu
NO_FRAME = RF.NO_FRAME
PAUSE, JOIN_S = RF.PAUSE, RF.JOIN_S
BIG = 1 << 16
MAXES = (0, 1, 3, BIG)                                                  # the staging blocks of a group grow when the first BIG arrives
# the forms of a group call: which of the two destination pointers the caller passes (cwslg_fetch_decodes has no report block)
FORMS = ("decodes", "reports", "reports_null_dec", "reports_null_rep")
SCHEDULED = RF.SCHEDULED


@pytest.fixture
def xctx():
    """A fresh context in the default (exact) arithmetic mode: the expected frames are the oracle's, bit for bit."""
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


# ---- the calls -----------------------------------------------------------------------------------------------------------------------------------
Got = collections.namedtuple("Got", "E n n_total n_ch dec rep")          # dec / rep: bytes of the n records, None where the pointer was null


def _group_call(ctx, mode, form, E, mx):
    """One group fetch through the C interface.  -> None (CWSLG_ERR_NO_FRAME), a Got, or an int: any other status."""
    import cwsl_digi_amd as P
    dec = np.zeros(max(mx, 1), DR.DECODE_DTYPE) if form != "reports_null_dec" else None
    rep = np.zeros(max(mx, 1), RR.REPORT_DTYPE) if form in ("reports", "reports_null_dec") else None
    t0, n, nt, nc = C.c_uint64(int(E)), C.c_int(-1), C.c_int(-1), C.c_int(-1)
    dp, rp = (None if a is None else a.ctypes.data for a in (dec, rep))
    if form == "decodes":
        rc = ctx.L.cwslg_fetch_decodes(ctx.h, P.GROUPS[mode], C.byref(t0), dp, mx, C.byref(n), C.byref(nt), C.byref(nc))
    elif mode == "FT8":
        rc = ctx.L.cwslg_fetch_decode_reports(ctx.h, P.GROUPS[mode], C.byref(t0), dp, rp, mx, C.byref(n), C.byref(nt), C.byref(nc))
    else:
        rc = ctx.L.cwslg_fetch_ft4_decode_reports(ctx.h, C.byref(t0), dp, rp, mx, C.byref(n), C.byref(nt), C.byref(nc))
    if rc == NO_FRAME:
        return None
    if rc != 0:
        return int(rc)
    k = max(n.value, 0)
    return Got(t0.value, n.value, nt.value, nc.value, None if dec is None else dec[:k].tobytes(), None if rep is None else rep[:k].tobytes())


def _first_record(got, want, size):
    for q in range(min(len(got), len(want)) // size):
        if got[q * size:(q + 1) * size] != want[q * size:(q + 1) * size]:
            return f"first differing record {q}: {got[q * size:(q + 1) * size].hex()}, expected {want[q * size:(q + 1) * size].hex()}"
    return f"{len(got) // size} records, expected {len(want) // size}"


class _GroupJudge:
    """The single rule for the group fetches; collects failures (a thread never raises), the epochs seen per mode and form, the statuses other
    than CWSLG_ERR_NO_FRAME, and how many calls came back empty-handed."""

    def __init__(self, config_at, n_epochs, chans):
        self.config_at, self.n_epochs, self.chans = config_at, n_epochs, chans      # chans: mode -> channel ids
        self.failures, self.statuses = [], []
        self.seen = collections.defaultdict(set)                        # (mode, form) -> epoch indices
        self.calls, self.nones = collections.Counter(), collections.Counter()
        self.fired = {m: None for m in chans}                           # the last boundary the clock has marked before firing it (epoch index it ends)
        self.done = {m: None for m in chans}                            # the last boundary that has returned
        self.lock = threading.Lock()

    def fail(self, text):
        self.failures.append(text)
        return False

    def runs(self, mode, e):
        return RC.chain_runs(mode, self.config_at(mode, e))

    def want(self, mode, e):
        return RC.group_expected(mode, e, self.config_at(mode, e), self.chans[mode])

    def may_be_empty(self, mode, done_before, fired_after):
        """The newest boundary the call can have met is one of done_before .. fired_after (None: none yet)."""
        if done_before is None:
            return True
        return any(not self.runs(mode, e) for e in range(done_before, (done_before if fired_after is None else fired_after) + 1))

    def check(self, mode, form, asked, mx, got, done_before=None, fired_after=None):
        """-> False after a failure (the consumer stops)."""
        where = f"{form}({mode}, E={asked}, max={mx})"
        with self.lock:
            self.calls[(mode, form)] += 1
            self.nones[(mode, form)] += got is None
        if isinstance(got, int):
            self.statuses.append((where, got))
            return self.fail(f"{where}: status {got}")
        if got is None:
            if asked == 0 and not self.may_be_empty(mode, done_before, fired_after):
                return self.fail(f"{where}: nothing to fetch although the boundaries of epochs {done_before} .. {fired_after} all ran the chain")
            return True
        e = RC.epoch_index(mode, got.E)
        if e is None or e >= self.n_epochs[mode]:
            return self.fail(f"{where}: stamped {got.E}, no epoch of this run")
        if asked and got.E != asked:
            return self.fail(f"{where}: stamped {got.E}, another epoch than the one asked for")
        cfg = self.config_at(mode, e)
        w = self.want(mode, e)
        if w is None:
            return self.fail(f"{where}: stamped {got.E} (epoch {e}, {cfg}), whose boundary ran without the chain")
        dec, rep, total = w
        if (got.n_ch, got.n_total, got.n) != (2, total, min(total, mx)):
            return self.fail(f"{where}: epoch {e}, {cfg}: n_channels {got.n_ch}, n_total {got.n_total}, n {got.n}; expected 2, {total}, {min(total, mx)}")
        for name, g, wnt, size in (("decodes", got.dec, dec, DR.DECODE_DTYPE.itemsize), ("reports", got.rep, rep, RR.REPORT_DTYPE.itemsize)):
            if g is not None and g != wnt[:got.n].tobytes():
                return self.fail(f"{where}: epoch {e}, {cfg}: the {name} are not that epoch's -- {_first_record(g, wnt[:got.n].tobytes(), size)}")
        self.seen[(mode, form)].add(e)
        return True

    def report(self, title, dt):
        seen = {f"{m} {f}": sorted(v) for (m, f), v in sorted(self.seen.items())}
        nones = {f"{m} {f}": f"{self.nones[(m, f)]} of {c}" for (m, f), c in sorted(self.calls.items())}
        print(f"\n{title}: {dt:.2f} s; epochs seen per call {seen}; calls that came back empty-handed {nones}")


def _group_round(ctx, judge, mode, form, mx):
    """One call with *start_epoch = 0 and, after a success, the same call with the explicit epoch it named: the same bytes or nothing."""
    done_before = judge.done[mode]
    got = _group_call(ctx, mode, form, 0, mx)
    fired_after = judge.fired[mode]
    if not judge.check(mode, form, 0, mx, got, done_before, fired_after):
        return False
    if got is not None:
        again = _group_call(ctx, mode, form, got.E, mx)
        if not judge.check(mode, form, got.E, mx, again):
            return False
        if again is not None and again != got:
            return judge.fail(f"{form}({mode}, max={mx}): asked again with E={got.E}, other bytes than the first time")
    return True


def _precompute(judge, modes):
    for mode in modes:
        for k in range(len(RC.RF[mode])):
            for e in range(judge.n_epochs[mode]):
                RC.expected(mode, k, e, judge.config_at(mode, e))
        for e in range(judge.n_epochs[mode]):
            judge.want(mode, e)


def _group_plan(mode):
    """Every form with every max, in an order that puts different forms and sizes next to each other."""
    return [(mode, form, MAXES[(i + j) % len(MAXES)]) for j in range(len(MAXES)) for i, form in enumerate(FORMS)]


# ---- a free-running clock ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", RC.MODES)
def test_group_fetches_race_a_free_running_clock(xctx, mode):
    """All stages on throughout.  A clock thread pushes each epoch's slot and fires the boundary while three consumers rotate over
    cwslg_fetch_decodes and the mode's report fetch -- with both blocks, without `dec`, without `rep` -- and over max = 0, 1, 3, 65536, each from
    another place of the rotation.  After every success the consumer asks again with the epoch it was given.  Once the first emitting
    boundary has returned, no call with *start_epoch = 0 may come back empty-handed; every form must have been seen at three or more epochs,
    the last included."""
    ctx, n = xctx, RC.N_RACE[mode]
    g = RF._open(ctx, [mode])[mode]
    g.configure(RC.ALL_ON)
    judge = _GroupJudge(lambda m, e: RC.ALL_ON, {mode: n}, {mode: g.chans})
    _precompute(judge, [mode])
    stop = threading.Event()

    def clock():
        try:
            g.boundary(0)
            for e in range(n):
                RF._push(ctx, g.rx, mode, e)
                judge.fired[mode] = e
                g.boundary(e + 1)
                judge.done[mode] = e
                time.sleep(PAUSE)
        except Exception as ex:       # pragma: no cover
            judge.fail(f"clock: {ex!r}")
        finally:
            stop.set()

    plan = _group_plan(mode)

    def consumer(first):
        try:
            left = None                                                 # once the clock has finished: one more whole rotation
            for i in itertools.count(first):
                if left is None and stop.is_set():
                    left = len(plan)
                if not _group_round(ctx, judge, *plan[i % len(plan)]):
                    return
                if left is not None:
                    left -= 1
                    if left == 0:
                        return
        except Exception as ex:       # pragma: no cover
            judge.fail(f"consumer: {ex!r}")

    t0 = time.monotonic()
    RF._run_threads(ctx, [threading.Thread(target=clock, name="clock")] +
                    [threading.Thread(target=consumer, args=(5 * j + 1,), name=f"consumer {j}") for j in range(3)])
    judge.report(f"{mode} group fetches against a free-running clock", time.monotonic() - t0)
    assert not judge.failures, judge.failures[:3]
    assert g.fired == n + 1
    for form in FORMS:
        assert n - 1 in judge.seen[(mode, form)] and len(judge.seen[(mode, form)]) >= 3, (form, sorted(judge.seen[(mode, form)]))


# ---- the schedules, single-threaded ------------------------------------------------------------------------------------------------------------------
_LAUNCHES = {}                                                          # "boundaries": stats.sync_launches after both schedules, no thread involved


def _walk_the_schedules(ctx, groups, after_boundary=None):
    """Both schedules step by step, as the clocks of the toggle test walk them.  -> stats.sync_launches at the end."""
    for mode in RC.MODES:
        groups[mode].configure(RC.SCHEDULE[mode][0])
        groups[mode].boundary(0)
    for e in range(max(RC.N_EPOCHS.values())):
        for mode in RC.MODES:
            if e < RC.N_EPOCHS[mode]:
                g = groups[mode]
                RF._push(ctx, g.rx, mode, e)
                g.configure(RC.SCHEDULE[mode][e])
                g.boundary(e + 1)
                if after_boundary:
                    after_boundary(mode, e)
    return ctx.stats()["sync_launches"]


def _boundary_launches():
    """What the boundaries of both schedules alone add to stats.sync_launches: taken from the late-consumer test when it has run in this
    process (it proves that no fetch moves the figure), otherwise from a walk without a single fetch in a context of its own."""
    if "boundaries" not in _LAUNCHES:
        import cwsl_digi_amd as P
        c = P.Context(0)
        try:
            _LAUNCHES["boundaries"] = _walk_the_schedules(c, RF._open(c, RC.MODES))
        finally:
            c.close()
    return _LAUNCHES["boundaries"]


def test_late_consumer_of_the_group_fetches(xctx):
    """Single-threaded.  Both schedules step by step: after every boundary every form of both group fetches, at every max, equals
    group_expected of that epoch under the step's configuration -- the cut list and OSD off included, compared here with values made on the
    CPU alone -- or hands out nothing where the step switched the chain off (then an explicit older epoch has nothing either).  No fetch moves
    stats.sync_launches.  After the last boundary two rounds of every call: the same bytes."""
    ctx = xctx
    groups = RF._open(ctx, RC.MODES)
    judge = _GroupJudge(SCHEDULED, dict(RC.N_EPOCHS), {m: groups[m].chans for m in RC.MODES})
    _precompute(judge, RC.MODES)

    def round_of(mode, e):
        out = []
        launches = ctx.stats()["sync_launches"]
        for _, form, mx in _group_plan(mode):
            for ask in (0, RC.start_epoch(mode, e)):
                got = _group_call(ctx, mode, form, ask, mx)
                assert judge.check(mode, form, ask, mx, got, e, e), judge.failures
                assert (got is None) == (not judge.runs(mode, e)), (mode, e, form, ask, mx)
                assert got is None or got.E == RC.start_epoch(mode, e), (mode, e, form, ask, got.E)
                out.append(got)
            if e > 0:                                                   # the epoch before is gone, whatever that boundary ran
                assert _group_call(ctx, mode, form, RC.start_epoch(mode, e - 1), mx) is None, (mode, e, form)
        assert ctx.stats()["sync_launches"] == launches
        return out

    t0 = time.monotonic()
    assert all(_group_call(ctx, m, f, 0, BIG) is None for m in RC.MODES for f in FORMS)      # nothing yet, before any boundary
    launches = _walk_the_schedules(ctx, groups, round_of)
    last = {m: RC.N_EPOCHS[m] - 1 for m in RC.MODES}
    first = [round_of(m, last[m]) for m in RC.MODES]
    again = [round_of(m, last[m]) for m in RC.MODES]
    assert first == again and all(got is not None for r in first for got in r)               # the last step has everything on
    assert ctx.stats()["sync_launches"] == launches
    _LAUNCHES["boundaries"] = launches
    judge.report("late consumer of the group fetches", time.monotonic() - t0)
    assert not judge.failures, judge.failures[:3]
    for mode in RC.MODES:                                               # every step that ran the chain was compared, in every form
        ran = {e for e in range(RC.N_EPOCHS[mode]) if judge.runs(mode, e)}
        assert all(judge.seen[(mode, form)] == ran for form in FORMS), (mode, ran, dict(judge.seen))


# ---- both groups, toggles, reallocation and a reloaded code --------------------------------------------------------------------------------------------
PER_CHANNEL = {"FT8": ("fetch_ft8_decode", "fetch_ft8_osd"), "FT4": ("fetch_ft4_sync", "fetch_ft4_osd")}      # they share the group's ticket


def test_both_groups_toggles_and_a_reloaded_code(xctx):
    """One context, an FT8 and an FT4 group, a clock thread per group that walks record_race_cases.SCHEDULE under the shared configuration
    lock (as in test_gpu_record_fetch_races.py): OSD off, decode off, (FT4: the coherent stage off,) the list cut to 5 and back, so that every
    boundary frees or reallocates what the previous epoch's late readers read.  Four consumers mix cwslg_fetch_decodes and the report fetch of
    BOTH groups (all forms, all sizes) with two per-channel record fetches per mode -- report_mu, the encoder's device copy and the two
    HarvestStage blocks meet only here.  A fifth thread reloads the SAME parity-check table once per PAUSE: the expected bytes do not change,
    and the encoder is uploaded again between report calls of both groups.  Both clocks finish; no status other than CWSLG_ERR_NO_FRAME is
    seen; every group call is seen at three or more epochs, the last included, the per-channel fetches at two or more; stats.sync_launches
    ends at what the boundaries alone account for."""
    ctx = xctx
    want_launches = _boundary_launches()
    groups = RF._open(ctx, RC.MODES)
    judge = _GroupJudge(SCHEDULED, dict(RC.N_EPOCHS), {m: groups[m].chans for m in RC.MODES})
    records = RF._Judge(SCHEDULED)
    _precompute(judge, RC.MODES)
    cfg_lock = threading.Lock()
    running = {m: threading.Event() for m in RC.MODES}
    both_done = lambda: all(ev.is_set() for ev in running.values())
    nm = LC.make_code(RC.SEED)["nm"]
    reloads = [0]

    def clock(mode):
        g = groups[mode]
        try:
            with cfg_lock:
                g.configure(RC.SCHEDULE[mode][0])
                g.boundary(0)
            for e in range(RC.N_EPOCHS[mode]):
                RF._push(ctx, g.rx, mode, e)
                with cfg_lock:
                    g.configure(RC.SCHEDULE[mode][e])
                    judge.fired[mode] = e
                    g.boundary(e + 1)
                    judge.done[mode] = e
                time.sleep(PAUSE)
        except Exception as ex:       # pragma: no cover
            judge.fail(f"{mode} clock: {ex!r}")
        finally:
            running[mode].set()

    def reloader():
        try:
            while not both_done():
                ctx.set_ldpc_code(nm)
                reloads[0] += 1
                time.sleep(PAUSE)
        except Exception as ex:       # pragma: no cover
            judge.fail(f"reloader: {ex!r}")

    plan = []
    for i in range(len(FORMS) * len(MAXES)):
        for mode in RC.MODES:
            plan.append(("group",) + _group_plan(mode)[i])
            name = PER_CHANNEL[mode][i % 2]
            k = (i // 2) % 2
            plan.append(("record", mode, k, groups[mode].chans[k], name))

    def consumer(first):
        try:
            left = None                                                 # once both clocks have finished: one more whole rotation
            for i in itertools.count(first):
                if left is None and both_done():
                    left = len(plan)
                step = plan[i % len(plan)]
                if step[0] == "group":
                    if not _group_round(ctx, judge, *step[1:]):
                        return
                else:
                    _, mode, k, ch, name = step
                    if not records.check(mode, k, name, RF._fetch(ctx, mode, name, ch)):
                        return
                if left is not None:
                    left -= 1
                    if left == 0:
                        return
        except Exception as ex:       # pragma: no cover
            judge.fail(f"consumer: {ex!r}")

    t0 = time.monotonic()
    RF._run_threads(ctx, [threading.Thread(target=clock, args=(m,), name=f"{m} clock") for m in RC.MODES] +
                    [threading.Thread(target=reloader, name="reloader")] +
                    [threading.Thread(target=consumer, args=(17 * j + 1,), name=f"consumer {j}") for j in range(4)])
    dt = time.monotonic() - t0
    judge.report(f"both groups, toggles and a reloaded code ({reloads[0]} reloads)", dt)
    records.report("   its per-channel record fetches", dt)
    assert not judge.statuses, judge.statuses[:3]
    assert not judge.failures and not records.failures, (judge.failures[:3], records.failures[:3])
    assert reloads[0] >= 3
    for mode in RC.MODES:
        assert groups[mode].fired == RC.N_EPOCHS[mode] + 1
        for form in FORMS:
            seen = judge.seen[(mode, form)]
            assert len(seen) >= 3 and RC.N_EPOCHS[mode] - 1 in seen, (mode, form, sorted(seen))
        for stage in ("msg", "osd") if mode == "FT8" else ("sync", "osd"):
            assert len(records.seen[(mode, stage)]) >= 2, (mode, stage, sorted(records.seen[(mode, stage)]))
    assert ctx.stats()["sync_launches"] == want_launches
