"""CPU: the slots of tests/harvest_twin_cases.py repeat words in every way tests/test_gpu_fetch_decodes.py::test_ft4_twins_against_the_cpu_chain
needs -- proved with the restatements alone (oracle.Channel -> FT4 candidates -> sync records -> soft bits -> ldpc_ref -> osd_ref ->
decodes_ref).  If a property is missing here the amplitudes, frequencies and seeds change, not the assertions."""
import decodes_ref as DR
import harvest_twin_cases as T


def _carriers(k, e):
    """word -> [(entry, by_osd, nharderr)] of one channel and slot, before de-duplication."""
    c = T.chain(k, e)
    out = {}
    for q in range(len(c["msg"])):
        w = DR._word_ft4(c["msg"][q], c["osd"][q])
        if w is not None and not DR.all_zero_word(w[2]):
            out.setdefault(w[2], []).append((q, w[0], w[3]))
    return out


def test_twin_slots_repeat_words_in_every_way():
    """Over the slots: a word on two BP records with unequal nharderr; a word on a BP and an OSD record of which the OSD record has the smaller
    entry, so that the entry reported is not the smallest carrier; a word on two OSD records; a word on three records.  Every word with more than
    one carrier is one that was sent, and the answer names the best carrier by (by_osd, nharderr, entry)."""
    two_bp_unequal = osd_before_bp = two_osd = three = winner_not_first = 0
    for e in range(T.N_EPOCHS):
        car = _carriers(0, e)
        sent = {T.sent_bits(t[3]) for t in T.TRANSMISSIONS[e]}
        assert sent <= set(car), e                                      # every message is decoded
        for word, lst in car.items():
            bp, osd = [(q, nh) for q, by, nh in lst if not by], [(q, nh) for q, by, nh in lst if by]
            assert len(lst) == 1 or word in sent
            two_bp_unequal += any(a[1] != b[1] for i, a in enumerate(bp) for b in bp[i + 1:])
            osd_before_bp += bool(bp) and bool(osd) and min(osd)[0] < min(bp)[0]
            two_osd += len(osd) >= 2
            three += len(lst) >= 3
        recs, n = T.expected([0, 1], e)
        mine = recs[recs["ch_id"] == 0]
        assert len(mine) == len(car) and sorted(bytes(r["bits"]) for r in mine) == sorted(car)
        for r in mine:
            lst = car[bytes(r["bits"])]
            assert (int(r["by_osd"]), int(r["nharderr"]), int(r["entry"])) == min((by, nh, q) for q, by, nh in lst) and int(r["ndup"]) == len(lst)
            winner_not_first += int(r["entry"]) != min(q for q, _, _ in lst)
    assert two_bp_unequal >= 1 and osd_before_bp >= 1 and two_osd >= 1 and three >= 1 and winner_not_first >= 2, \
        (two_bp_unequal, osd_before_bp, two_osd, three, winner_not_first)
    assert max(int(T.expected([0, 1], e)[0]["ndup"].max()) for e in range(T.N_EPOCHS)) >= 3


def test_noise_channel_has_a_list_and_at_most_osd_finds():
    for e in range(T.N_EPOCHS):
        c = T.chain(1, e)
        assert len(c["list"]) > 0 and len(c["sync"]) > 0
        assert all(by for lst in _carriers(1, e).values() for _, by, _ in lst)            # no word by BP in noise


def test_slots_differ_and_osd_matters():
    """The slots give different answers (a stale generation is visible), and without OSD fewer decodes come out of a slot or a worse carrier is
    named."""
    full = [T.expected([0, 1], e)[0].tobytes() for e in range(T.N_EPOCHS)]
    assert len(set(full)) == T.N_EPOCHS
    assert all(T.expected([0, 1], e, osd=False)[0].tobytes() != full[e] for e in range(T.N_EPOCHS))
    assert any(T.expected([0, 1], e, osd=False)[1] < T.expected([0, 1], e)[1] for e in range(T.N_EPOCHS))
    assert all(len(T.chain(0, e)["list"]) < T.MAX_CAND for e in range(T.N_EPOCHS))           # the limit cuts nothing
