"""CPU: the signal recipes of tests/softbits_cases.py do what tests/test_gpu_softbits_scale.py assumes, shown on the reference alone.

Every recipe's IQ goes through the oracle's own chain (oracle.Channel(mode, 48000, 1024, dial).push_many(iq) and .boundary(...)), then through
the oracle's searches and the numpy restatements (tests/ft8_softbits_ref.py, tests/ft4_softbits_ref.py).  The conditions are the ones the GPU
module asserts again on the library's output (softbits_cases.assert_ft8_found, assert_ft4_found, assert_no_foreign_record and the counts below):
  1  every probe burst is found with nsync 16 (FT4) / 21 (FT8) and no wrong sign in set 0;
  2  the edge recipe yields records with f1_hz < 260 and > 4700;
  3  the dense recipe yields more than 200 FT8 entries at syncmin 1.2;
  4  the max_cand 7 recipe's full lists are longer than 7;
  5  the many-then-few pairs have strictly fewer entries in the second slot;
  6  no probe channel of the 37-channel recipe holds a record with sync > 2.5 at another probe's frequency.
A recipe that misses its condition is changed (amplitude, start time, frequency), never the condition.

Cost: 70 frames through the oracle and the restatements, about 40 s on one core in total."""
import numpy as np
import pytest

import ft8_softbits_ref as R8
import softbits_cases as S


def _ft8(oracle, iq, dial, max_cand=200, f_hi=3000, syncmin=1.5, order="sync"):
    fr = S.oracle_frame(oracle, "FT8", dial, iq)
    cands = oracle.ft8_sync(fr, 200, f_hi, syncmin, max_cand, order=order)
    return fr, cands, S.ft8_reference(oracle, fr, cands, R8.soft_pitch(f_hi))


def _ft4(oracle, iq, dial, split=None, max_cand=100, f_lo=200, f_hi=3000, order="sync"):
    fr = S.oracle_frame(oracle, "FT4", dial, iq, split)
    cands = oracle.ft4_candidates(fr, float(f_lo), float(f_hi), 1.2, max_cand, order=order)
    return fr, cands, S.ft4_reference(oracle, fr, cands)


def _pair_found(oracle, iq, tones, ft8, ft4, f_hi=3000):
    """Every burst of every channel of one pair slot is found (condition 1)."""
    for dial, bursts in ft8:
        _, cands, r = _ft8(oracle, iq, dial, max_cand=100, f_hi=f_hi)
        S.assert_ft8_found(cands, r["llr"], r["nsync"], bursts, tones[("FT8", dial)])
    for dial, bursts in ft4:
        _, _, r = _ft4(oracle, iq, dial, split=S.N4, f_hi=f_hi)
        S.assert_ft4_found(r["recs"], r["llr"], r["nsync"], bursts, tones[("FT4", dial)])


def test_many_channels_recipe(oracle):
    """Conditions 1 and 6 on the six probes; the two noise-only channels hold no strong record at any probe's frequency."""
    iq, tones = S.many_channels_iq(oracle)
    starts = set()
    for p, bursts in S.MANY_PROBES.items():
        _, _, r = _ft4(oracle, iq, S.MANY_DIALS[p])
        S.assert_ft4_found(r["recs"], r["llr"], r["nsync"], bursts, tones[("FT4", S.MANY_DIALS[p])])
        S.assert_no_foreign_record(r["recs"], p)
        starts |= {(b[0], b[1]) for b in bursts}
    assert len(starts) == sum(len(b) for b in S.MANY_PROBES.values()) and len({a for a, _ in starts}) == len(starts)     # every probe its own frequencies and start times
    for k in S.MANY_NOISE_ONLY:
        _, _, r = _ft4(oracle, iq, S.MANY_DIALS[k])
        S.assert_no_foreign_record(r["recs"], None)


@pytest.mark.parametrize("k", [0, 1, 2])
def test_both_features_recipe(oracle, k):
    seed, ft8, ft4 = S.both_slot(k)
    iq, tones = S.pair_iq(oracle, seed, ft8, ft4)
    _pair_found(oracle, iq, tones, ft8, ft4, f_hi=2959)                      # the GPU test runs this recipe with f_hi = 2959


@pytest.mark.parametrize("k", range(6))
def test_reconfigure_recipe(oracle, k):
    """Condition 1 under the configuration of slot k; condition 4 at slot 1."""
    seed, ft8, ft4 = S.reconf_slot(k)
    max_cand, f_hi, order = S.RECONF_CONFIG[k]
    iq, tones = S.pair_iq(oracle, seed, ft8, ft4)
    (d8, b8), (d4, b4) = ft8[0], ft4[0]
    fr8, cands, r = _ft8(oracle, iq, d8, max_cand=max_cand, f_hi=f_hi, order=order)
    S.assert_ft8_found(cands, r["llr"], r["nsync"], b8[:2], tones[("FT8", d8)][:2])
    fr4, c4, r4 = _ft4(oracle, iq, d4, split=S.N4, max_cand=max_cand, f_hi=f_hi, order=order)
    S.assert_ft4_found(r4["recs"], r4["llr"], r4["nsync"], b4[:2], tones[("FT4", d4)][:2])
    if max_cand == 7:
        assert len(cands) == 7 and len(oracle.ft8_sync(fr8, 200, f_hi, 1.5, 200)) > 7
        assert len(c4) == 7 and len(oracle.ft4_candidates(fr4, 200.0, float(f_hi), 1.2, 100)) > 7


@pytest.mark.parametrize("k", [0, 1, 2])
def test_open_and_close_recipe(oracle, k):
    seed, _, _, ft8, ft4 = S.churn_slot(k)
    iq, tones = S.pair_iq(oracle, seed, ft8, ft4)
    _pair_found(oracle, iq, tones, ft8, ft4)


def test_list_recipes(oracle):
    """The four-signal channel (full list longer than 3), the dense one (condition 3) and the many-then-few pairs (condition 5)."""
    d8, d4 = S.LISTS_FT8_DIAL, S.LISTS_FT4_DIAL
    iq, tones = S.build_iq(oracle, 340, S.N8, ft8=[(d8, S.LISTS_FOUR)])
    _, cands, r = _ft8(oracle, iq, d8, max_cand=600)
    assert len(cands) > 3
    S.assert_ft8_found(cands, r["llr"], r["nsync"], S.LISTS_FOUR, tones[("FT8", d8)])
    iq, _ = S.build_iq(oracle, 341, S.N8, ft8=[(d8, S.LISTS_DENSE)])
    fr = S.oracle_frame(oracle, "FT8", d8, iq)
    assert 200 < len(oracle.ft8_sync(fr, 200, 3000, 1.2, 600)) < 600
    n8, n4 = [], []
    for seed, b8, b4 in ((342, S.LISTS_MANY8, S.LISTS_MANY4), (343, S.LISTS_FEW8, S.LISTS_FEW4)):
        iq, tones = S.pair_iq(oracle, seed, [(d8, b8)], [(d4, b4)])
        _, cands, r = _ft8(oracle, iq, d8)
        n8.append(len(cands))
        if len(b8) == 1:
            S.assert_ft8_found(cands, r["llr"], r["nsync"], b8, tones[("FT8", d8)])
        _, c4, r4 = _ft4(oracle, iq, d4, split=S.N4, max_cand=200)
        n4.append((len(c4), len(r4["recs"])))
        if len(b4) == 1:
            S.assert_ft4_found(r4["recs"], r4["llr"], r4["nsync"], b4, tones[("FT4", d4)])
    assert 1 <= n8[1] < n8[0], n8
    assert 1 <= n4[1][0] < n4[0][0] and 1 <= n4[1][1] < n4[0][1], n4


def test_band_edge_recipe(oracle):
    """Conditions 1 and 2 with the search open from 100 to 5000 Hz."""
    iq, tones = S.build_iq(oracle, 350, S.N4, ft4=[(S.EDGE_DIAL, S.EDGE_BURSTS)])
    _, cands, r = _ft4(oracle, iq, S.EDGE_DIAL, f_lo=100, f_hi=5000)
    f1 = [h["f1_hz"] for h in r["recs"]]
    assert min(f1) < 260 and max(f1) > 4700, (min(f1), max(f1))
    S.assert_ft4_found(r["recs"], r["llr"], r["nsync"], S.EDGE_BURSTS, tones[("FT4", S.EDGE_DIAL)])
    q_lo, q_hi = S.ft4_best(r["recs"], S.EDGE_BURSTS[0]), S.ft4_best(r["recs"], S.EDGE_BURSTS[1])
    assert r["recs"][q_lo]["f1_hz"] < 260 and r["recs"][q_hi]["f1_hz"] > 4700          # the decoded edge bursts ARE the edge records


def test_ticket_recipe(oracle):
    iq, tones = S.pair_iq(oracle, 360, S.TICKET_FT8, S.TICKET_FT4)
    _pair_found(oracle, iq, tones, S.TICKET_FT8, S.TICKET_FT4)
    _, cands, _ = _ft8(oracle, iq, S.TICKET_FT8[0][0])
    _, _, r = _ft4(oracle, iq, S.TICKET_FT4[0][0], split=S.N4)
    assert len(cands) >= 3 and len(r["recs"]) >= 3                                       # three records of each kind to recompute
