"""CPU: the inputs of the a-priori GPU tests are what they are for -- the mixed batch reaches every exit of the kernel, the slot of the fetch
test contains every case the fetch has to handle (proved on the CPU chain: the oracle's frames, then the restatements of every stage) -- and what
a-priori decoding is WORTH against this chain's own BP + OSD, measured with the restatements alone (never against the GPU); only the direction
is asserted, the figures go to DESIGN.md 4.12 and profiles/ft8_ap_cost.json."""
import json
import os

import numpy as np
import pytest

import ap_cases as C
import ap_ref as AP
import decodes_ref as DR
import ldpc_cases as LC
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O

CODE = LC.make_code(C.SEED)["code"]


def test_the_batch_reaches_every_exit():
    llr, sent = C.batch()
    for n_pat in C.BATCH_NPAT:
        rec = C.batch_reference(n_pat)
        m = rec["msg"]
        assert (m["iters"] == -1).sum() == 2 and set(np.nonzero(m["iters"] == -1)[0]) == {100, 201}             # not finite: not attempted
        found = np.nonzero(m["crc_ok"] == 1)[0]
        assert set(m["pad_"][found]) <= set(range(n_pat)) and set(range(min(n_pat, 5))) <= set(m["pad_"][found])       # every known field finds
        assert (m["pad_"][m["crc_ok"] == 0] == 0xff).all() and (rec["dmin"][m["crc_ok"] == 0] == 0).all()
        assert n_pat == 1 or ((m["crc_ok"] == 0) & (m["iters"] > C.MAX_ITER)).any()                         # a sum over several runs
        for q in found:                                                                                     # never a wrong word on a transmission
            if sent[q] is not None and not DR.all_zero_word(m["bits"][q]):
                assert np.array_equal(R.unpack_bits(m["bits"][q]), sent[q]), q
    # the all-zero sets succeed under pattern 3 (a field of zeros) once it is among the patterns, with the all-zero word
    rec8 = C.batch_reference(8)
    zeros = [q for q in range(C.BATCH_N) if not llr[q].any()]
    assert zeros and all(rec8["msg"]["pad_"][q] == 3 and not rec8["msg"]["bits"][q].any() for q in zeros)
    assert all(C.batch_reference(2)["msg"]["crc_ok"][q] == 0 for q in zeros)


def test_noisy_seed_is_what_the_rule_cases_say():
    """second_right / no_success: BP and OSD order 2 both miss the word, the right pattern finds it."""
    pat, x, word = C.rule_cases()["second_right"]
    assert R.decode(CODE, x[None], C.MAX_ITER)[0]["crc_ok"] == 0
    assert O.decode(OC.generator(C.SEED), x[None], 2)[0]["crc_ok"] == 0
    r = AP.decode(CODE, x[None], pat[1:], C.MAX_ITER)[0]
    assert r["msg"]["crc_ok"] == 1 and np.array_equal(R.unpack_bits(r["msg"]["bits"]), word)


# ---- the slot of the fetch test -----------------------------------------------------------------------------------------------------------------
def _words(rec):
    return {q: rec["bits"][q].tobytes() for q in range(len(rec)) if rec["crc_ok"][q]}


def test_the_slot_contains_every_case():
    A, B, Cw, D, E = (C.bits12(m) for m in (C.MSG_A, C.MSG_B, C.MSG_C, C.MSG_D, C.MSG_E))
    c0 = C.slot_chain(0)
    bp, osd, ap, ap_no = _words(c0["msg"]), _words(c0["osd"]), _words(c0["ap"]["msg"]), _words(c0["ap_no_osd"]["msg"])
    pad = c0["ap"]["msg"]["pad_"]
    assert set(bp.values()) == {A, B} and set(osd.values()) == {B}
    # BP and OSD both fail, the a-priori pass finds the transmitted word: under pattern 0 (A) and under a later one (C, E)
    assert not (set(ap) & (set(bp) | set(osd)))
    assert sorted(ap.values()) == sorted([A, Cw, E, E])
    assert {pad[q] for q, w in ap.items() if w == A} == {0} and {pad[q] for q, w in ap.items() if w in (Cw, E)} == {1}
    assert A in bp.values()                                             # the a-priori word A is a BP word of another entry: the merge helper's case
    # with OSD off at the boundary the entry OSD decoded is attempted, and pattern 0 finds its word
    (q_osd,) = osd
    assert q_osd not in ap and ap_no[q_osd] == B and c0["ap_no_osd"]["msg"]["pad_"][q_osd] == 0
    assert {q: w for q, w in ap_no.items() if q != q_osd} == ap
    # what the fetch hands out for the channel: E once with ndup 2; by_osd, set and dmin of the a-priori record
    where = DR.where_ft8(c0["list"])
    rec, total = C.ap_decodes([(7, where, c0["ap"])])
    assert total == 3 and [r["bits"].tobytes() for r in rec] == sorted([A, Cw, E], key=lambda w: min(q for q, x in ap.items() if x == w))
    e = rec[[r["bits"].tobytes() for r in rec].index(E)]
    assert e["ndup"] == 2 and e["by_osd"] == 2 and e["set"] == 1 and e["dmin"] == c0["ap"]["dmin"][e["entry"]] > 0 and (rec["ch_id"] == 7).all()
    # the list cut at 5 keeps both entries of E and nothing else of the a-priori words; cut at 1 there is none
    c5 = C.slot_chain(0, 5)
    assert sorted(_words(c5["ap"]["msg"]).values()) == [E, E]
    assert not _words(C.slot_chain(0, 1)["ap"]["msg"])
    # a channel with a decode and no a-priori find; a channel of noise
    c1 = C.slot_chain(1)
    assert set(_words(c1["msg"]).values()) == {D} and not _words(c1["ap"]["msg"]) and (c1["ap"]["msg"]["iters"] > 0).any()
    for k in (2, 3, 4):
        c = C.slot_chain(k)
        assert not _words(c["msg"]) and not _words(c["ap"]["msg"]) and not _words(c["ap_no_osd"]["msg"]) and len(c["list"]) > 0


def test_merge_helper_keeps_bp_and_osd_words():
    from cwsl_digi_amd.api import merge_ap_decodes
    c0 = C.slot_chain(0)
    where = DR.where_ft8(c0["list"])
    dec, _ = DR.decodes("FT8", [(7, where, c0["msg"], c0["osd"])])
    ap, _ = C.ap_decodes([(7, where, c0["ap"])])
    merged = merge_ap_decodes(dec, ap)
    A = C.bits12(C.MSG_A)
    assert len(merged) == len(dec) + len(ap) - 1                        # A is dropped from the a-priori words: BP has it
    assert [m["by_osd"] for m in merged if m["bits"].tobytes() == A] == [0]
    assert list(merged["entry"]) == sorted(merged["entry"]) and set(merged["by_osd"]) == {0, 2}     # (B: BP on one entry, OSD on another -- one BP decode)
    assert merge_ap_decodes(dec, ap[:0]).tobytes() == dec.tobytes()


# ---- what a-priori decoding is worth ------------------------------------------------------------------------------------------------------------
WORTH_NOISE = (0.7, 0.8, 0.9, 1.0)          # around BP's 50 % point under this code with ldpc_cases' scaling
WORTH_N = 48                                # transmissions per level
NOISE_N = 250                               # noise-only sets x 4 patterns = 1000 trials


def test_what_ap_is_worth(tmp_path):
    G = OC.generator(C.SEED)
    pats = C.patterns(4)
    out = dict(code_seed=int(C.SEED), max_iter=C.MAX_ITER, osd_order=2, known_bits=C.NPRE, n_patterns=4, transmissions_per_level=WORTH_N, levels=[])
    extra, wrong = 0, 0
    for noise in WORTH_NOISE:
        sent = [C.message(20000 + q, C.PREFIXES[q % 4]) for q in range(WORTH_N)]
        llr = np.stack([C.noisy(C.SEED, sent[q], noise, 500 + q) for q in range(WORTH_N)])
        bits = [C.bits12(m) for m in sent]
        bp = R.decode(CODE, llr, C.MAX_ITER)
        osd = O.decode(G, llr, 2, bp["crc_ok"] == 0)
        ap = AP.decode(CODE, llr, pats, C.MAX_ITER, (bp["crc_ok"] == 0) & (osd["crc_ok"] == 0))
        ok_bp = np.array([bool(bp["crc_ok"][q]) and bp["bits"][q].tobytes() == bits[q] for q in range(WORTH_N)])
        ok_osd = ok_bp | np.array([bool(osd["crc_ok"][q]) and osd["bits"][q].tobytes() == bits[q] for q in range(WORTH_N)])
        ok_ap = np.array([bool(ap["msg"]["crc_ok"][q]) and ap["msg"]["bits"][q].tobytes() == bits[q] for q in range(WORTH_N)])
        wrong += int((ap["msg"]["crc_ok"] == 1).sum() - ok_ap.sum())
        extra += int((ok_ap & ~ok_osd).sum())
        out["levels"].append(dict(noise=noise, bp=float(ok_bp.mean()), bp_osd=float(ok_osd.mean()), bp_osd_ap=float((ok_osd | ok_ap).mean()),
                                  osd_wrong=int(((osd["crc_ok"] == 1).sum() + (bp["crc_ok"] == 1).sum()) - ok_osd.sum())))
    rng = np.random.default_rng(99)
    noise_llr = (np.float32(2.83) * rng.standard_normal((NOISE_N, R.N))).astype(np.float32)
    false = 0
    for p in range(4):                                                   # every pattern on its own: sets x patterns trials
        r = AP.decode(CODE, noise_llr, pats[p:p + 1], C.MAX_ITER)
        false += int(sum(1 for q in range(NOISE_N) if r["msg"]["crc_ok"][q] and not DR.all_zero_word(r["msg"]["bits"][q])))
    out["false_finds_per_1000"] = 1000.0 * false / (4 * NOISE_N)
    print(json.dumps(out))
    dst = os.environ.get("CWSLG_AP_WORTH_JSON")
    if dst:
        with open(dst, "w") as fh:
            json.dump(out, fh, indent=1)
    assert extra >= 1, "a-priori decoding found nothing that BP + OSD missed"
    assert wrong == 0, "a-priori decoding returned a wrong word on a transmission that carries the pattern"
    for lv in out["levels"]:
        assert lv["bp"] <= lv["bp_osd"] <= lv["bp_osd_ap"]
