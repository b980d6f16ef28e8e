"""CPU: oracle restatement vs the compiled reference headers (oracle/_ref), through what they returned for the inputs of
tests/ref_cases.py: tests/golden/ref_*.npz, recorded by `python tests/gen_golden.py ref` where the reference can be built."""
import hashlib
import os

import numpy as np
import pytest

import ref_cases as RC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gold(name):
    with np.load(os.path.join(GOLD, name)) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def misc():
    return _gold("ref_misc.npz")


@pytest.mark.parametrize("fs,f,usb", RC.DEMOD_CASES)
def test_bit_identical_audio_and_phasor(oracle, fs, f, usb):
    g = _gold(RC.demod_file(fs, f, usb))
    a, ta = oracle.Demod(fs, float(f), usb=usb).run(RC.demod_iq(oracle, fs, f, usb), trace=True)
    assert np.array_equal(a.view(np.uint32), g["audio_bits"])
    assert np.array_equal(ta.view(np.uint64), g["trace_bits"])


def test_getters_and_errors(oracle, misc):
    in_size, out_size, out_rate, delay, ntaps, block = (int(x) for x in misc["getters_192k"])
    assert (in_size, out_size, out_rate, delay) == (64, 4, 12000, 8)
    d = oracle.Demod(192000, 0.0)
    assert (d.ntaps, d.block, 4 * d.block) == (ntaps, block, in_size)
    for args, want, msg in zip(RC.BAD_DEMODS, misc["bad_demod_errors"], ("low", "high", None)):
        with pytest.raises(ValueError) as e2:
            oracle.Demod(*args)
        assert str(e2.value) == str(want)
        if msg:
            assert msg in str(want)
    assert str(misc["bad_demod_errors"][2]) == "Fs/B must be an even integer >= 4"


def test_lowpass_design_matches(oracle, misc):
    for k, (order, bw) in enumerate(RC.LOWPASS_CASES):
        a = np.empty(order, np.float32)
        oracle.lib().orc_lowpass_design(order, bw, a)
        assert np.array_equal(a.view(np.uint32), misc[f"lowpass_{k}_bits"])


# ---- slot framing: the oracle's Channel against Instance's sequences replayed on the reference's own containers ----
@pytest.mark.parametrize("mode,fs,blk,f", RC.FRAMING_CASES)
def test_framing_matches_reference_containers(oracle, mode, fs, blk, f):
    """Random schedules of blocks and boundaries, including over-full slots ("af buffer full"), empty slots and the
    discarded first frame: same drop decisions, same epochs, same sample counts, bit-identical float frames."""
    g = _gold(RC.framing_file(mode, fs, blk, f))
    oc = oracle.Channel(mode, fs, blk, f)
    assert oc.frame_len == oracle.frame_len(mode)
    took, n_emit = [], 0
    for slot, (blocks, epoch) in enumerate(RC.framing_schedule(oracle, mode, fs, blk, f)):
        took += [oc.push(b) for b in blocks]
        fo = oc.boundary(epoch, want_f32=True)
        assert (fo is not None) == bool(g["emitted"][slot])
        if fo is not None:
            assert fo["t_start"] == int(g["t_start"][slot])
            assert np.array_equal(fo["f32"][:1024].view(np.uint32), g["frame_head_bits"][n_emit])
            assert hashlib.sha256(fo["f32"].view(np.uint32).tobytes()).hexdigest() == str(g["frame_sha256"][n_emit])
            n_emit += 1
    assert took == [int(t) for t in g["took"]]
    n_drop = len(took) - sum(took)
    assert n_emit == 5 and n_drop >= 5                           # first frame discarded; the over-full slot dropped blocks


def test_mode_groups_match_syncpredicates(misc):
    import cwsl_digi_amd as P
    for m, g in zip(RC.MODES, misc["mode_groups"]):
        if m == "PSK31":
            assert g == -1
            continue
        assert g == P.group_of(m) == P.parse_decoder_line(f"14074000 {m}", 1.0)["group"], m
    with pytest.raises(Exception):
        P.parse_decoder_line("14074000 PSK31", 1.0)


def test_locator_and_trim_helpers_match_reference(oracle, misc):
    import cwsl_digi_amd as P
    locs, padded = RC.helper_strings()
    assert locs == [str(x) for x in misc["locators"]]
    for loc, valid in zip(locs, misc["locator_valid"]):
        line = f"123045 -12  0.3 1234 ~  CQ K1ABC {loc}"
        got = P.parse_decode_line("FT8", line, 0)
        want = oracle.parse_decode_line("FT8", line, 0)
        assert got == want
        if got["status"] == "ok" and got["call"] == "K1ABC":
            assert (got["locator"] is not None) == bool(valid), loc
    for line, trimmed in zip(padded, misc["trimmed"]):
        assert str(trimmed) == RC.TRIM_CORE
        assert P.parse_decode_line("FT8", line, 0)["call"] == "K1ABC"


def test_tune_on_a_live_demodulator_matches_reference(oracle, misc):
    """SSBD::Tune(F, isUSB) mid-stream: the oracle's orc_demod_tune against the compiled header, incl. a rejected retune."""
    fs, iq, n1, f0, bad, f1 = RC.tune_live_case(oracle)
    a = oracle.Demod(fs, f0)
    ya = a.run(iq[:n1])
    assert np.array_equal(ya.view(np.uint32), misc["tune_live_bits_0"])
    with pytest.raises(ValueError, match=r"Signal outside of band \(high\)"):
        a.tune(bad)                                           # |F + B| > Fs/2: thrown before anything is stored
    assert str(misc["tune_live_error"]) == "Signal outside of band (high)"
    a.tune(f1)
    ya = a.run(iq[n1:])
    assert np.array_equal(ya.view(np.uint32), misc["tune_live_bits_1"])
    assert np.array_equal(a.tone.view(np.uint32), misc["tune_live_tone_bits"])
    # a retuned object equals a freshly constructed one from that point on (workspace, index and phase are reset)
    c = oracle.Demod(fs, f1)
    assert np.array_equal(c.run(iq[n1:]).view(np.uint32), ya.view(np.uint32))


def test_tune_without_reset_matches_reference(oracle, misc):
    """SSBD::Tune(F, isUSB, reset = false) (SSBD.hpp:97,116-121): workspace, index and phase survive the retune.  The oracle's
    orc_demod_tune_ex against the compiled header, bit for bit, through two retunes (one of them flipping the sideband)."""
    fs, iq, f0, cuts, plan = RC.tune_noreset_case(oracle)
    a = oracle.Demod(fs, f0)
    outs = []
    for k in range(3):
        if plan[k] is not None:
            a.tune(plan[k][0], plan[k][1], reset=False)
        ya = a.run(iq[cuts[k]:cuts[k + 1]])
        assert np.array_equal(ya.view(np.uint32), misc[f"tune_noreset_bits_{k}"]), k
        outs.append(ya)
    # and it is NOT the reset form: the 31 outputs after the retune still carry the old tuning's partial sums
    c = oracle.Demod(fs, f0)
    c.run(iq[:cuts[1]]); c.tune(60000, True, reset=True)
    yc = c.run(iq[cuts[1]:cuts[2]])
    assert not np.array_equal(yc[:31].view(np.uint32), outs[1][:31].view(np.uint32))
