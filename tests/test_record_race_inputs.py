"""CPU: the inputs of tests/test_gpu_record_fetch_races.py, checked with the restatements alone before any GPU sees them -- the conditions that keep
the race tests from hiding a failure: in every channel and every stage any two epochs differ (a stale or a mixed generation is always visible),
every list is non-empty and within its limit and is really cut at the smaller limit, every epoch has OSD records that were attempted and others
that were not, and in some epochs OSD returns a word where belief propagation had none.  For tests/test_gpu_report_fetch_races.py the same of
the group fetches: the totals per epoch, decodes of both channels at every scheduled boundary that runs the chain, any two epochs different in
decodes and in reports, a scheduled step that changes them, no report on its floor.  If a property is missing the inputs in
tests/record_race_cases.py change, not these assertions."""
import numpy as np
import pytest

import ft4_osd_cases as X
import ldpc_ref as R
import record_race_cases as RC


def _epochs(mode):
    return range(RC.N_EPOCHS[mode])


@pytest.mark.parametrize("mode", RC.MODES)
def test_any_two_epochs_differ_in_every_stage(mode):
    for k in range(len(RC.RF[mode])):
        for stage in RC.STAGES[mode]:
            seen = {RC.expected(mode, k, e)[stage] for e in _epochs(mode)}
            assert None not in seen and len(seen) == RC.N_EPOCHS[mode], (mode, k, stage)
        # ... and under the configuration the toggle schedule puts each epoch under: what ran differs from every OTHER epoch's records with
        # everything on, which is what a buffer that was not rewritten or a stamp that was not reset would hand out
        for e in _epochs(mode):
            exp = RC.expected(mode, k, e, RC.SCHEDULE[mode][e])
            for stage in RC.STAGES[mode]:
                if exp[stage] is not None:
                    assert all(exp[stage] != RC.expected(mode, k, o)[stage] for o in _epochs(mode) if o != e), (mode, k, e, stage)


@pytest.mark.parametrize("mode", RC.MODES)
def test_lists_are_within_their_limit_and_the_smaller_limit_cuts_them(mode):
    cut = [e for e in _epochs(mode) if RC.SCHEDULE[mode][e].max_cand == RC.CUT_CAND]
    assert cut
    for k in range(len(RC.RF[mode])):
        for e in _epochs(mode):
            n = len(RC.chain(mode, k, e, RC.MAX_CAND)["list"])
            assert 1 <= n <= RC.MAX_CAND
            assert RC.uncut_list_length(mode, k, e) > RC.CUT_CAND
        for e in cut:
            c = RC.chain(mode, k, e, RC.CUT_CAND)
            assert len(c["list"]) == RC.CUT_CAND
            exp = RC.expected(mode, k, e, RC.SCHEDULE[mode][e])
            assert all(exp[s] is not None and exp[s] != RC.expected(mode, k, e)[s] for s in RC.STAGES[mode] if s != "frame")
            if mode == "FT4":
                assert 1 <= len(c["sync"]) <= 3 * RC.CUT_CAND and len(c["msg"]) == len(c["osd"]) == len(c["sync"])


def _osd_attempted(mode, osd):
    return osd["how"] != 0xff if mode == "FT8" else X.attempted(osd).any(axis=1)


@pytest.mark.parametrize("mode", RC.MODES)
def test_every_epoch_has_osd_records_of_both_kinds(mode):
    for k in range(len(RC.RF[mode])):
        for e in _epochs(mode):
            for max_cand in {RC.MAX_CAND, RC.SCHEDULE[mode][e].max_cand}:
                att = _osd_attempted(mode, RC.chain(mode, k, e, max_cand)["osd"])
                assert att.any() and (~att).any(), (mode, k, e, max_cand)


@pytest.mark.parametrize("mode", RC.MODES)
def test_osd_returns_words_belief_propagation_had_not(mode):
    """RECOVERED's weak transmissions: no record has the sent bits from belief propagation, one has them from OSD with crc_ok -- inside the epochs
    of the free-running tests and in both."""
    assert RC.RECOVERED[mode] and all(e < RC.N_RACE[mode] for e, _ in RC.RECOVERED[mode])
    for e, k in RC.RECOVERED[mode]:
        c = RC.chain(mode, k, e, RC.MAX_CAND)
        sent = RC.message(RC.transmissions(mode, e, k)[1][3])
        msg, osd = c["msg"], c["osd"]
        if mode == "FT8":
            assert not any(m["crc_ok"] and np.array_equal(R.unpack_bits(m["bits"]), sent) for m in msg)
            hits = [q for q in range(len(osd)) if osd[q]["crc_ok"] and np.array_equal(R.unpack_bits(osd[q]["bits"]), sent)]
            assert hits and all(msg[q]["iters"] >= 1 and msg[q]["crc_ok"] == 0 for q in hits), (e, k)
        else:
            hits = X.find_word(msg, osd, sent)
            assert hits and all(by_osd for _, by_osd in hits), (e, k)
            assert not (msg["set"]["crc_ok"][[q for q, _ in hits]] != 0).any()


def test_a_stage_that_is_off_has_nothing_to_hand_out():
    for mode in RC.MODES:
        on = RC.expected(mode, 0, 0)
        assert all(on[s] is not None for s in RC.STAGES[mode])
        no_osd = RC.expected(mode, 0, 0, RC.ALL_ON._replace(osd=False))
        assert no_osd["osd"] is None and all(no_osd[s] == on[s] for s in RC.STAGES[mode] if s != "osd")
        no_msg = RC.expected(mode, 0, 0, RC.ALL_ON._replace(decode=False))
        assert no_msg["osd"] is None and no_msg["msg"] is None and no_msg["soft"] == on["soft"]
        no_soft = RC.expected(mode, 0, 0, RC.ALL_ON._replace(soft=False))
        assert no_soft["osd"] is None and no_soft["msg"] is None and no_soft["soft"] is None and no_soft["list"] == on["list"]
    off = RC.expected("FT4", 0, 0, RC.ALL_ON._replace(coherent=False))
    assert [s for s in RC.STAGES["FT4"] if off[s] is None] == ["sync", "soft", "msg", "osd"] and off["list"] == RC.expected("FT4", 0, 0)["list"]
    assert RC.expected("FT8", 0, 0, RC.ALL_ON._replace(coherent=False)) == RC.expected("FT8", 0, 0)


# ---- the group fetches (tests/test_gpu_report_fetch_races.py) ---------------------------------------------------------------------------------------
IDS = (0, 1)
NO_OSD, CUT = RC.ALL_ON._replace(osd=False), RC.ALL_ON._replace(max_cand=RC.CUT_CAND)
TOTALS = {("FT8", RC.ALL_ON): (2, 3, 3, 3, 2, 3), ("FT8", NO_OSD): (2, 2, 2, 2, 2, 3), ("FT8", CUT): (2, 3, 3, 3, 2, 3),
          ("FT4", RC.ALL_ON): (10, 6, 9, 9, 6, 10, 4), ("FT4", NO_OSD): (9, 6, 8, 8, 5, 8, 3)}
BY_OSD = {"FT8": (1, 2, 3), "FT4": (0, 2, 3, 4, 5, 6)}                    # the epochs with a by_osd decode, everything on
FLOOR_DB = {"FT8": -24.0, "FT4": -21.0}


def test_group_totals():
    """n_total of group_expected per epoch, as measured with the restatements when the race tests were written."""
    for (mode, cfg), want in TOTALS.items():
        assert tuple(RC.group_expected(mode, e, cfg, IDS)[2] for e in _epochs(mode)) == want, (mode, cfg)
    assert RC.group_expected("FT4", 5, CUT, IDS)[2] == 7
    for mode in RC.MODES:
        assert tuple(e for e in _epochs(mode) if RC.group_expected(mode, e, RC.ALL_ON, IDS)[0]["by_osd"].any()) == BY_OSD[mode]


@pytest.mark.parametrize("mode", RC.MODES)
def test_every_scheduled_boundary_that_runs_the_chain_gives_decodes_of_both_channels(mode):
    ran = 0
    for e in _epochs(mode):
        cfg = RC.SCHEDULE[mode][e]
        g = RC.group_expected(mode, e, cfg, IDS)
        assert (g is None) == (not RC.chain_runs(mode, cfg))
        if g is not None:
            dec, rep, n_total = g
            assert len(dec) == len(rep) == n_total >= (2 if mode == "FT8" else 4) and set(dec["ch_id"].tolist()) == set(IDS), (mode, e, n_total)
            ran += 1
    assert ran >= 4
    g = RC.group_expected(mode, 0, RC.ALL_ON, (7, 9))                   # the channel ids are the caller's
    assert set(g[0]["ch_id"].tolist()) == {7, 9} and g[1].tobytes() == RC.group_expected(mode, 0, RC.ALL_ON, IDS)[1].tobytes()


@pytest.mark.parametrize("mode", RC.MODES)
def test_group_bytes_of_any_two_epochs_differ(mode):
    """Decodes and reports alike, with everything on and under the schedule: a stale or a mixed generation is always visible."""
    for which in (0, 1):
        on = [RC.group_expected(mode, e, RC.ALL_ON, IDS)[which].tobytes() for e in _epochs(mode)]
        assert len(set(on)) == len(on), (mode, which)
        for e in _epochs(mode):
            g = RC.group_expected(mode, e, RC.SCHEDULE[mode][e], IDS)
            if g is not None:
                assert all(g[which].tobytes() != on[o] for o in _epochs(mode) if o != e), (mode, which, e)


@pytest.mark.parametrize("mode", RC.MODES)
def test_a_cut_list_or_osd_off_changes_the_group_bytes_of_a_scheduled_epoch(mode):
    """In each mode a scheduled step other than "all on" hands out other decodes AND other reports than everything on would at that epoch.
    (Measured: FT8 the OSD-off step, epoch 1; FT4 the cut list, epoch 5.  The FT8 cut of epoch 4 keeps both decodes among its five candidates and
    the FT4 OSD-off step of epoch 1 has no OSD word to lose: there the expected bytes are those of everything on.)"""
    changed = []
    for e in _epochs(mode):
        cfg = RC.SCHEDULE[mode][e]
        g = RC.group_expected(mode, e, cfg, IDS)
        if cfg != RC.ALL_ON and g is not None:
            on = RC.group_expected(mode, e, RC.ALL_ON, IDS)
            if g[0].tobytes() != on[0].tobytes() and g[1].tobytes() != on[1].tobytes():
                changed.append(e)
    assert changed, mode


@pytest.mark.parametrize("mode", RC.MODES)
def test_no_report_sits_on_its_floor(mode):
    """A report at the floor is the value a kernel that read nothing (or noise alone) would also give."""
    for e in _epochs(mode):
        for cfg in {RC.ALL_ON, NO_OSD, CUT, RC.SCHEDULE[mode][e]}:
            g = RC.group_expected(mode, e, cfg, IDS)
            if g is not None and g[2]:
                rep = g[1]
                assert (rep["snr_db"] > FLOOR_DB[mode]).all() and (rep["xsig"] > 0).all() and (rep["xnoise"] > 0).all(), (mode, e, cfg, rep)


def test_epochs_records_and_the_description_of_a_difference():
    for mode in RC.MODES:
        assert [RC.epoch_index(mode, RC.start_epoch(mode, e)) for e in range(RC.N_EPOCHS[mode])] == list(range(RC.N_EPOCHS[mode]))
        assert RC.epoch_index(mode, RC.start_epoch(mode, 0) + 1) is None and RC.epoch_index(mode, RC.start_epoch(mode, RC.N_EPOCHS[mode])) is None
        assert RC.N_RACE[mode] <= RC.N_EPOCHS[mode] == len(RC.SCHEDULE[mode])
        for stage in RC.STAGES[mode][1:]:
            a, b = RC.expected(mode, 0, 0)[stage], RC.expected(mode, 0, 1)[stage]
            rb = RC.record_bytes(mode, stage)
            assert len(a) % rb == 0 and len(a) > 0
            assert RC.first_difference(mode, stage, a, a) == "" and "first differing record " in RC.first_difference(mode, stage, a, b)
            assert RC.first_difference(mode, stage, a[:-rb], a) == f"{len(a) // rb - 1} records, expected {len(a) // rb}"
    from cwsl_digi_amd import api
    assert RC.CAND_DTYPE.itemsize == 20 and RC.SYNC4_DTYPE.itemsize == 32
    assert RC.record_bytes("FT8", "msg") == api.FT8_MSG_DTYPE.itemsize and RC.record_bytes("FT4", "msg") == api.FT4_MSG_DTYPE.itemsize
    assert RC.record_bytes("FT8", "osd") == api.OSD_MSG_DTYPE.itemsize and RC.record_bytes("FT4", "osd") == api.FT4_OSD_DTYPE.itemsize
