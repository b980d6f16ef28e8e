"""CPU: the inputs of tests/test_gpu_record_fetch_races.py, checked with the restatements alone before any GPU sees them -- the conditions that keep
the race tests from hiding a failure: in every channel and every stage any two epochs differ (a stale or a mixed generation is always visible),
every list is non-empty and within its limit and is really cut at the smaller limit, every epoch has OSD records that were attempted and others
that were not, and in some epochs OSD returns a word where belief propagation had none.  If a property is missing the inputs in
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
