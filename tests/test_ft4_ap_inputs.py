"""CPU: the slots of tests/test_gpu_fetch_ft4_ap.py contain what they were made for -- proved on the CPU chain (the oracle's frames, then
ft4_softbits_ref, ft4_decode_cases, ft4_osd_cases, ft4_ap_ref, decodes_ref) -- and what a-priori decoding is WORTH on the FT4 chain against its
own BP + OSD, measured with the restatements alone (never against the GPU): only the direction is asserted, the figures go to DESIGN.md 4.13."""
import json
import os

import numpy as np

import ap_cases as APC
import decodes_ref as DR
import ft4_ap_cases as F
import ft4_ap_ref as A4
import ldpc_cases as LC

CODE = LC.make_code(F.SEED)["code"]


def _finds(ap):
    """[(entry, set, pattern, bits)] of every set with an a-priori find."""
    m = ap["set"]["msg"]
    return [(q, s, int(m["pad_"][q, s]), m["bits"][q, s].tobytes()) for q in range(len(ap)) for s in range(3) if m["crc_ok"][q, s]]


def _words(rec):
    return {(q, s): rec["set"]["bits"][q, s].tobytes() for q in range(len(rec)) for s in range(3) if rec["set"]["crc_ok"][q, s]}


def test_the_starved_slot():
    rec, total = F.expected("starved")
    assert total == len(rec) >= 6 and (rec["by_osd"] == 2).all()
    s, p = rec["set"] & 3, rec["set"] >> 2
    assert (s != 0).any() and (p != 0).any() and set(p) <= {0, 1, 2} and (rec["ndup"] == 2).sum() == 1 and (rec["dmin"] > 0).any()
    assert set(rec["ch_id"]) == {0, 1}                                  # the third channel hears noise: records, attempts, no find
    for k in range(3):
        c, ap = F.records("starved", k), F.ap_records("starved", k)
        assert c["osd"] is None and len(c["msg"]) > 0
        sent = F.sent("starved", k)
        assert all(b in sent for _, _, _, b in _finds(ap))             # never a word that was not sent
        taken = A4.taken(c["msg"], None, c["soft"]["nsync"], c["soft"]["nqual"], *F.SETTINGS["starved"][2])
        att = ap["set"]["msg"]["iters"] >= 0
        assert (att.any(axis=1) == taken).all() and taken.any() and not taken.all()
        # the a-priori minima lie above the decode's: a record the decode attempted and the a-priori gate leaves
        assert ((c["msg"]["set"]["iters"] >= 0).any(axis=1) & ~(c["msg"]["set"]["crc_ok"] != 0).any(axis=1) & ~taken).any()
        if k == 2:
            assert not _finds(ap) and (ap["set"]["msg"]["iters"] > F.AP_MAX_ITER).any()      # a sum over several patterns' runs
    # one record BP did decode, starved as it is, is not attempted
    c0, ap0 = F.records("starved", 0), F.ap_records("starved", 0)
    bp = sorted({q for q, s in _words(c0["msg"])})
    assert bp and (ap0["set"]["msg"]["iters"][bp] == -1).all()
    assert len(bp) < len(F.TX["starved"][0]) / 2                         # BP fails on most transmissions
    # with the empty mask alone the answer differs: a known field finds a word in an earlier set than the plain pass does (the choice is set-major)
    one, total1 = F.expected("starved", n_pat=1)
    assert 0 < total1 <= total and (one["set"] >> 2 == 0).all() and (one["set"] & 3).sum() > (rec["set"] & 3).sum()
    # the lists are cut inside a candidate's records at 1 and 4, and the cut changes the answer
    assert F.expected("starved", max_cand=4)[1] < total
    assert len(F.records("starved", 2, 1)["sync"]) <= 3 and len(F.records("starved", 2)["list"]) == F.MAX_CAND


def test_the_normal_slot():
    c0, c1 = F.records("normal", 0), F.records("normal", 1)
    ap, ap_no = F.ap_records("normal", 0), F.ap_records("normal", 0, osd=False)
    sent = F.sent("normal", 0)
    bp, osd = _words(c0["msg"]), _words(c0["osd"])
    finds = _finds(ap)
    # records BP and OSD miss in all sets, found by the a-priori pass under both patterns
    assert len(finds) >= 1 and {p for _, _, p, _ in finds} == {0, 1} and all(b in sent for *_, b in finds)
    have = {q for q, s in bp} | {q for q, s in osd}
    assert not ({q for q, *_ in finds} & have)
    assert not (set(b for *_, b in finds) & (set(bp.values()) | set(osd.values())))
    # a record OSD decodes is attempted only with OSD off at the boundary
    q_osd = sorted({q for q, s in osd} - {q for q, s in bp})
    assert q_osd and (ap["set"]["msg"]["iters"][q_osd] == -1).all() and (ap_no["set"]["msg"]["iters"][q_osd] >= 0).any()
    a1, a1_no = F.ap_records("normal", 1), F.ap_records("normal", 1, osd=False)
    assert not _finds(a1) and _finds(a1_no) and {b for *_, b in _finds(a1_no)} <= set(_words(c1["osd"]).values())
    rec, total = F.expected("normal")
    rec_no, total_no = F.expected("normal", osd=False)
    assert 1 <= total < total_no and set(rec["ch_id"]) == {0} and set(rec_no["ch_id"]) == {0, 1}
    assert not _finds(F.ap_records("normal", 2)) and len(F.records("normal", 2)["msg"]) > 0


def test_merge_helper_on_ft4_records():
    from cwsl_digi_amd.api import merge_ap_decodes
    ch = [(k, DR.where_ft4(F.records("normal", k)["sync"]), F.records("normal", k)["msg"], None) for k in range(3)]
    dec, _ = DR.decodes("FT4", ch)                                        # the boundary's words with OSD off
    ap, _ = F.expected("normal", osd=False)
    merged = merge_ap_decodes(dec, ap)
    assert len(merged) == len(dec) + len(ap) and set(merged["by_osd"]) == {0, 2}
    assert [tuple(x) for x in merged[["ch_id", "entry"]].tolist()] == sorted(tuple(x) for x in merged[["ch_id", "entry"]].tolist())
    twice = merge_ap_decodes(merged[merged["by_osd"] == 0], np.concatenate([ap, ap[:1]]))
    assert len(twice) == len(merged) + 1                                 # (the helper merges against BP / OSD words only)
    own = dec[:1].copy()
    own["by_osd"], own["set"] = 2, 1 | 2 << 2
    assert merge_ap_decodes(dec, own).tobytes() == dec.tobytes()       # a word BP already has on the channel is dropped


# ---- what a-priori decoding is worth ------------------------------------------------------------------------------------------------------------
def test_what_ap_is_worth():
    pats = F.patterns("normal")
    mins = F.SETTINGS["normal"][2]
    out = dict(code_seed=int(F.SEED), max_iter=F.AP_MAX_ITER, osd_order=2, known_bits=29, n_patterns=len(pats), sigma=F.SIGMA,
               transmissions_per_level=len(F.WORTH_SEEDS) * len(F.WORTH_HZ), levels=[])
    extra = wrong = false = trials = 0
    for lv, amp in enumerate(F.WORTH_AMPS):
        n_bp = n_osd = n_ap = 0
        for seed in F.WORTH_SEEDS:
            c, noise = F.worth_slot(lv, seed)
            ap = A4.decode(CODE, c["soft"], c["msg"], c["osd"], pats, F.AP_MAX_ITER, *mins)
            f1 = np.array([r["f1_hz"] for r in c["sync"]])
            sent = [APC.bits12(F.worth_message(lv, seed, j)) for j in range(len(F.WORTH_HZ))]
            for j, hz in enumerate(F.WORTH_HZ):
                near = np.nonzero(np.abs(f1 - hz) <= 4.0)[0]
                ok_bp = any(w == sent[j] for (q, s), w in _words(c["msg"]).items() if q in near)
                ok_osd = ok_bp or any(w == sent[j] for (q, s), w in _words(c["osd"]).items() if q in near)
                ok_ap = any(b == sent[j] for q, s, p, b in _finds(ap) if q in near)
                n_bp, n_osd, n_ap = n_bp + ok_bp, n_osd + ok_osd, n_ap + (ok_osd or ok_ap)
                extra += ok_ap and not ok_osd
            wrong += sum(1 for *_, b in _finds(ap) if b not in sent and not DR.all_zero_word(b))
            # noise-only records behind the gate x 3 sets, every pattern on its own
            for p in range(len(pats)):
                a = A4.decode(CODE, noise["soft"], noise["msg"], noise["osd"], pats[p:p + 1], F.AP_MAX_ITER, *mins)
                trials += int((a["set"]["msg"]["iters"] >= 0).sum())
                false += sum(1 for *_, b in _finds(a) if not DR.all_zero_word(b))
        n = len(F.WORTH_SEEDS) * len(F.WORTH_HZ)
        se = lambda k: float(np.sqrt(k / n * (1 - k / n) / n))
        out["levels"].append(dict(amplitude=amp, bp=n_bp / n, bp_osd=n_osd / n, bp_osd_ap=n_ap / n, se_bp=se(n_bp), se_bp_osd=se(n_osd), se_bp_osd_ap=se(n_ap)))
    out.update(ap_only=int(extra), wrong_words_in_the_transmission_slots=int(wrong), noise_trials=int(trials), false_finds_in_noise=int(false))
    print(json.dumps(out))
    dst = os.environ.get("CWSLG_FT4_AP_WORTH_JSON")
    if dst:
        with open(dst, "w") as fh:
            json.dump(out, fh, indent=1)
    for lv in out["levels"]:
        assert lv["bp"] <= lv["bp_osd"] <= lv["bp_osd_ap"]
    assert trials > 0
