"""CPU: the recipes of tests/degenerate_cases.py put before the kernels what tests/test_gpu_degenerate_frames.py assumes, shown on the reference
alone.

Every recipe's IQ goes through the oracle's own chain (oracle.Channel at 48 kHz, blocks of 1024, dial 0), then through every restatement in
order (degenerate_cases.reference) under both configurations.  Asserted per recipe (degenerate_cases.assert_conditions, which the GPU module
calls again on the library's output):
  zeros, impulse      the frame as described, both lists empty;
  carrier_on, FT8     the list full at 200, at least 100 repeated bit patterns in red[ia..ib], sigma below 0.01 and above 1e4, an all-zero word
                      with crc_ok at open gates;
  carrier_on, FT4     the top candidate's sync above 1e10, records in segments 1, 2 and 3;
  carrier_off         no FT8 candidate at all (the carrier sits between two bins), three FT4 sync records or more;
  dc                  frame maximum 0, the FT8 list full, the FT4 list empty;
  midslot             the FT4 first-half frame all zero while the FT8 list is full;
  clean8 / clean4     the strongest record decodes the message sent with nsync 21 / 16; FT8: report above 25 dB, 100 exact-zero LLRs or more;
  cut8_*              5000 exact-zero LLRs or more;   cut4_*: 30 or more, records in all three segments;
  blocker8 / blocker4 the weak message is decoded; FT8: max |llr| above 1000;
  comb, FT4, open     100 records or more, 50 all-zero words or more, none of them among decodes_ref's decodes.
  FT4 reports         (test_ft4_reports_of_the_recipes) clean4 and blocker4 one decode each with nsync 16 and nsymerr 0, 16.0 dB and above 8 dB;
                      cut4_tail 7 decodes, 2 of them by OSD alone, 5 on records with ibest < 0, nsymerr 22..27, nsync 9 or 10; cut4_head one
                      OSD-only decode with nsymerr 29; no FT4 decode anywhere else; every xsig and xnoise finite and positive.
A recipe that misses its condition is changed, never the condition.

No NaN and no infinity in any restatement's output -- with ONE exception, found while this module was written and pinned here: the baseline
array of getcandidates4 (the `red2` plane of cwslg_sync_debug_fetch on an FT4 channel) is NaN over the search range for an ALL-ZERO frame
(degenerate_cases.NAN_ALLOWED says why); no record, list or plane holds one.

The sensitivity tests show that the recipes cannot pass a kernel that gets a hazard wrong: each of three wrong rules changes expected bytes.

Cost: 30 frames, 60 chains and the ordinary slot's four; about 65 s on one core, most of it the numpy OSD at open gates."""
import numpy as np
import pytest

import decodes_ref as DR
import degenerate_cases as G
import ft8_softbits_ref as R8
import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O
from ft8_signal import ICOS7

MODES = ("FT8", "FT4")


def _ref(oracle, name, mode, cfg):
    return G.reference(oracle, mode, G.recipe_frame(name, mode), cfg)


@pytest.mark.parametrize("cfg", [G.UPSTREAM, G.OPEN], ids=lambda c: c.name)
@pytest.mark.parametrize("name", list(G.RECIPES))
def test_recipe_conditions(oracle, name, cfg):
    for mode in MODES:
        ref = _ref(oracle, name, mode, cfg)
        G.assert_conditions(name, mode, cfg, ref)
        assert len(ref["list"]) <= G.MAX_CAND[mode] and len(ref["msg"]) == len(ref["osd"]) == len(ref["llr"])
        for stage, a in G.stage_floats(ref).items():
            bad = ~np.isfinite(a)
            if (name, mode, stage) in G.NAN_ALLOWED:
                assert np.isnan(a[bad]).all() and bad.any() and not bad[:38].any() and not bad[577:].any(), (name, mode, stage)
            else:
                assert not bad.any(), (name, mode, stage, int(bad.sum()))


def test_every_recipe_is_in_one_group():
    names = [n for g in G.GROUPS.values() for n in g]
    assert sorted(names) == sorted(G.RECIPES) and len(set(names)) == len(names)
    assert {n for n, _ in G.ZERO_FRAMES} <= set(G.RECIPES)
    for name, mode in G.ZERO_FRAMES:
        assert not G.recipe_frame(name, mode).any()


@pytest.mark.parametrize("cfg", [G.UPSTREAM, G.OPEN], ids=lambda c: c.name)
def test_ordinary_slot(oracle, cfg):
    """The slot before and after the recipes: every burst found; the FT4 frame of the first half (noise alone) has a list of its own."""
    _, tones = G.ordinary()
    for mode in MODES:
        ref = G.reference(oracle, mode, G.ordinary_frame(mode), cfg)
        G.assert_ordinary(mode, ref, tones)
        assert all(np.isfinite(a).all() for a in G.stage_floats(ref).values())


# ---- what the recipes give the FT4 report ----------------------------------------------------------------------------------------------------------
FT4_DECODING = ("clean4", "blocker4", "cut4_tail", "cut4_head")


@pytest.mark.parametrize("cfg", [G.UPSTREAM, G.OPEN], ids=lambda c: c.name)
def test_ft4_reports_of_the_recipes(oracle, cfg):
    """cwslg_fetch_ft4_decode_reports meets, through the library, exactly the decodes its kernel has not met elsewhere: records with ibest < 0
    (leading symbols exact zeros, which tie to tone 0), OSD-only words, noise-free transmissions.  Measured with the restatements, identical
    under both configurations; the reports cost under 0.1 s per recipe."""
    got = {}
    for name in G.RECIPES:
        ref = _ref(oracle, name, "FT4", cfg)
        dec, rep = G.ft4_reports(ref)
        assert len(rep) == len(dec) and np.isfinite(rep["xsig"]).all() and np.isfinite(rep["xnoise"]).all() and np.isfinite(rep["snr_db"]).all()
        assert (rep["xsig"] > 0).all() and (rep["xnoise"] > 0).all(), (name, rep)
        if name not in FT4_DECODING:
            assert len(dec) == 0, (name, dec)
        got[name] = (ref, dec, rep)
    for name, floor in (("clean4", None), ("blocker4", 8.0)):
        _, dec, rep = got[name]
        assert len(dec) == 1 and not dec["by_osd"][0] and (rep["nsync"][0], rep["nsymerr"][0]) == (16, 0), (name, dec, rep)
        assert abs(float(rep["snr_db"][0]) - 16.0) < 0.05 if floor is None else rep["snr_db"][0] > floor, (name, rep)
    ref, dec, rep = got["cut4_tail"]
    early = [int(ref["recs"][int(q)]["ibest"]) < 0 for q in dec["entry"]]
    assert len(dec) == 7 and int(dec["by_osd"].sum()) == 2 and sum(early) == 5, (dec, early)
    assert rep["nsymerr"].min() >= 22 and rep["nsymerr"].max() <= 27 and set(rep["nsync"].tolist()) == {9, 10}, rep
    _, dec, rep = got["cut4_head"]
    assert len(dec) == 1 and dec["by_osd"][0] and rep["nsymerr"][0] == 29, (dec, rep)
    # the first halves the GPU module puts through the FT4 group fetch with the GPU's own records, and the ordinary slot: no FT4 decode
    frames = [G.oracle_frame(oracle, "FT4", G.recipe_iq(n), 0) for n in ("cut4_tail", "cut4_head")]
    frames += [G.oracle_frame(oracle, "FT4", G.ordinary()[0], 0), G.ordinary_frame("FT4")]
    for fr in frames:
        assert len(G.ft4_reports(G.reference(oracle, "FT4", fr, cfg))[0]) == 0


# ---- sensitivity: a wrong rule changes expected bytes ----------------------------------------------------------------------------------------------
def test_last_maximum_changes_nsync(oracle):
    """nsync with the LAST maximum of the eight tones instead of the first, from ft8_softbits_ref.magnitudes: a row of eight equal magnitudes (a
    symbol in digital silence) then names tone 7, never a Costas tone, where the first maximum names tone 0, which the Costas arrays contain."""
    changed = []
    for name in ("cut8_tail", "cut8_head", "clean8", "midslot"):
        ref = _ref(oracle, name, "FT8", G.UPSTREAM)
        s8 = R8.magnitudes(ref["plane"], ref["list"])[:, R8.COSTAS_SYMBOLS, :]
        last = 7 - np.argmax(s8[:, :, ::-1], axis=2)
        nsync_last = (last == np.array(ICOS7 * 3).reshape(1, -1)).sum(axis=1).astype(np.int32)
        first = (np.argmax(s8, axis=2) == np.array(ICOS7 * 3).reshape(1, -1)).sum(axis=1).astype(np.int32)
        assert np.array_equal(first, ref["nsync"])
        changed.append(int((nsync_last != ref["nsync"]).sum()))
    assert all(n > 0 for n in changed), changed


def test_dropping_the_zero_word_rule_changes_the_decodes(oracle, monkeypatch):
    for name, mode in (("comb", "FT4"), ("carrier_on", "FT8"), ("clean8", "FT8")):
        ref = _ref(oracle, name, mode, G.OPEN)
        want, total = DR.decodes(mode, [G.decodes_of(mode, 0, ref)])
        with monkeypatch.context() as m:
            m.setattr(DR, "all_zero_word", lambda bits: False)
            wrong, wrong_total = DR.decodes(mode, [G.decodes_of(mode, 0, ref)])
        assert wrong_total > total and wrong.tobytes() != want.tobytes(), (name, total, wrong_total)


def test_plus_zero_taken_as_one_changes_the_records(oracle):
    """The hard decision of an exact +0 LLR taken as 1: stated by replacing every +0 with the smallest positive float32 (1.4e-45: `> 0` holds, no
    sum or product it enters can tell it from zero).  The decode records (nharderr counts llr > 0 against the word) and the OSD records (the hard
    decisions are its starting word) of the first records of a cut slot change."""
    ref = _ref(oracle, "cut8_tail", "FT8", G.OPEN)
    n = 24
    llr = np.array(ref["llr"][:n])
    assert (llr == 0).sum() >= 100 and not np.signbit(llr[llr == 0]).any()
    llr[llr == 0] = np.float32(1.4e-45)
    code, Gm = C.make_code(G.SEED)["code"], OC.generator(G.SEED)
    msg = R.hard_records(code, llr, G.OPEN.max_iter, ref["nsync"][:n], ref["sigma"][:n], 0)
    assert msg.tobytes() != ref["msg"][:n].tobytes()
    osd = O.chain_records(Gm, llr, G.OPEN.order, ref["nsync"][:n], ref["msg"][:n], 0)
    assert osd.tobytes() != ref["osd"][:n].tobytes()
