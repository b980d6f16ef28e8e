"""CPU: the slots of tests/harvest_cases.py contain what tests/test_gpu_fetch_decodes.py needs them to contain -- proved with the restatements
alone (oracle.Channel -> ft8_sync / ft4 chain -> soft bits -> ldpc_ref -> osd_ref -> decodes_ref).  If a property is missing here the slots
change (message seeds, start steps), not the assertions."""
import numpy as np

import decodes_ref as DR
import harvest_cases as H
import record_race_cases as RC


def _carriers(mode, k, e, max_cand):
    """word -> [(entry, by_osd, nharderr)] of one channel and slot, before de-duplication."""
    c = H.chain(mode, k, e, max_cand)
    out = {}
    for q in range(len(c["msg"])):
        w = (DR._word_ft8 if mode == "FT8" else DR._word_ft4)(c["msg"][q], c["osd"][q])
        if w is not None and not DR.all_zero_word(w[2]):
            out.setdefault(w[2], []).append((q, w[0], w[3]))
    return out


def test_ft8_slots_repeat_words_in_every_way():
    """Over the FT8 slots: a word on two BP entries with equal nharderr; a word on a BP and an OSD entry; a decode that exists by OSD alone; a
    channel with a list and no decode.  And every strong transmission is decoded, as the word that was sent."""
    two_bp_equal = bp_and_osd = osd_only = list_without_decode = two_bp_unequal = 0
    for e in range(H.N_EPOCHS):
        car = _carriers("FT8", 0, e, H.MAX_CAND)
        for audio, t0, amp, mseed in H.transmissions8(e):
            if amp == H.AMP:
                assert H.sent_bits(mseed) in car, (e, mseed)
        for lst in car.values():
            bp = [(q, nh) for q, by, nh in lst if not by]
            two_bp_equal += any(a[1] == b[1] for i, a in enumerate(bp) for b in bp[i + 1:])
            two_bp_unequal += any(a[1] != b[1] for i, a in enumerate(bp) for b in bp[i + 1:])
            bp_and_osd += bool(bp) and len(bp) < len(lst)
            osd_only += not bp
        recs, n = H.expected("FT8", [0, 1], e, H.MAX_CAND, only=[0])
        assert n == len(car) and sorted(bytes(r["bits"]) for r in recs) == sorted(car)
        for r in recs:                                                  # the representative, restated: BP first, then the fewer hard errors, then the smaller entry
            assert (int(r["by_osd"]), int(r["nharderr"]), int(r["entry"])) == min((by, nh, q) for q, by, nh in car[bytes(r["bits"])])
            assert int(r["ndup"]) == len(car[bytes(r["bits"])])
        quiet = H.chain("FT8", 1, e, H.MAX_CAND)
        list_without_decode += len(quiet["list"]) > 0 and H.expected("FT8", [0, 1], e, H.MAX_CAND, only=[1])[1] == 0
    assert two_bp_equal >= 1 and two_bp_unequal >= 1 and bp_and_osd >= 1 and osd_only >= 1 and list_without_decode >= 1, \
        (two_bp_equal, two_bp_unequal, bp_and_osd, osd_only, list_without_decode)


def test_ft8_slots_differ_and_cut_lists_differ_too():
    """Any two slots give different answers (a stale generation is visible), and so do the list limits 1, 5 and 100 of one slot."""
    full = [H.expected("FT8", [0, 1], e, H.MAX_CAND)[0].tobytes() for e in range(H.N_EPOCHS)]
    assert len(set(full)) == H.N_EPOCHS
    for e in range(H.N_EPOCHS):
        n = [H.expected("FT8", [0, 1], e, mc)[1] for mc in (1, 5, 100)]
        assert n[0] == 1 and n[0] < n[1] <= n[2], n
    assert any(H.expected("FT8", [0, 1], e, H.MAX_CAND, osd=False)[1] < H.expected("FT8", [0, 1], e, H.MAX_CAND)[1] for e in range(H.N_EPOCHS))


def test_ft4_slots():
    """record_race_cases' first three FT4 slots: decodes on both channels in every slot, words from a set other than 0, a word by OSD -- and no
    word on two sync records: none is found in these slots nor in the recipe family of ft4_decode_cases (one burst moved through the slot in
    0.1 s steps at two amplitudes).  FT4 de-duplication runs on the GPU on the slots of tests/harvest_twin_cases.py, which send one message at
    several audio frequencies, and on the synthetic records of tests/harvest_kernel_cases.py."""
    sets, by_osd, dups = set(), 0, 0
    for e in range(H.N_EPOCHS):
        for k in range(2):
            recs, n = H.expected("FT4", [0, 1], e, RC.MAX_CAND, only=[k])
            assert n >= 2
            sets |= set(int(s) for s in recs["set"])
            by_osd += int(recs["by_osd"].sum())
            dups += int((recs["ndup"] > 1).sum())
            assert any(len(v) for v in _carriers("FT4", k, e, RC.MAX_CAND).values())
    assert sets >= {0, 1} and by_osd >= 1 and dups == 0
    full = [H.expected("FT4", [0, 1], e, RC.MAX_CAND)[0].tobytes() for e in range(H.N_EPOCHS)]
    assert len(set(full)) == H.N_EPOCHS
