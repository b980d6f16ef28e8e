"""CPU: the cases of tests/ft4_report_kernel_cases.py contain what tests/test_gpu_ft4_report_kernel.py says they contain -- proved on the case
data and on the restatement's answers alone -- and the case file is one the check program's vetting accepts."""
import numpy as np

import ft4_decode_reports_ref as R4
import ft4_report_kernel_cases as K

F32 = np.float32


def _case(name):
    return next(c for c in K.cases() if c["name"] == name)


def _reports(case):
    n = min(case["n_total"], case["lim"])
    return K.answer(case)[:K.REP_WORDS * n].view(R4.REPORT_DTYPE)


def _slots(ch):
    """slot of every entry of a channel: the nrec walk over min(cnt, cap) candidates"""
    n = min(ch["cnt"], ch["cap"])
    return [3 * k + r for k in range(n) for r in range(int(ch["nrec"][k]))]


def test_every_case_is_one_the_check_program_accepts():
    names = [c["name"] for c in K.cases()]
    assert len(set(names)) == len(names)
    for c in K.cases():
        off = c["offsets"]
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all() and len(off) == len(c["channels"])
        n = min(c["n_total"], c["lim"])
        for ch in c["channels"]:
            assert 1 <= ch["cap"] <= 600 and ch["cnt"] >= 0 and ch["nrec"].min() >= 0 and ch["nrec"].max() <= 3 and ch["spectrum"] in K.SPECTRA
            assert len(ch["sync"]) >= len(_slots(ch))
        for p, d in enumerate(c["records"][:n]):
            k = int(np.searchsorted(off, p, side="right")) - 1
            assert d["ch_id"] == 100 + k and 0 <= d["entry"] < len(_slots(c["channels"][k])), (c["name"], p)
            # the restatement reads the entry's record where the kernel's walk finds it
            ch = c["channels"][k]
            s = _slots(ch)[int(d["entry"])]
            assert ch["rec"][s // 3, s % 3]["f1_hz"] == ch["sync"][int(d["entry"])]["f1_hz"] and ch["rec"][s // 3, s % 3]["ibest"] == ch["sync"][int(d["entry"])]["ibest"]


def test_decode_counts_and_limits():
    assert [min(_case(f"decodes_{n}")["n_total"], _case(f"decodes_{n}")["lim"]) for n in (1, 2, 3, 5)] == [1, 2, 3, 5]
    lo, hi = _case("limit_below_total"), _case("limit_above_total")
    assert lo["lim"] < lo["n_total"] and len(lo["records"]) >= lo["lim"] and hi["lim"] > hi["n_total"]


def test_600_candidates_cross_the_passes_and_end_in_the_last_slot():
    c = _case("candidates_600")
    ch = c["channels"][0]
    assert ch["cap"] == ch["cnt"] == 600 and set(int(v) for v in ch["nrec"]) == {0, 1, 2, 3}
    slots = _slots(ch)
    hit = [slots[int(d["entry"])] for d in c["records"]]
    cands = [s // 3 for s in hit]
    assert 3 * 599 + 2 in hit                                            # the last slot of the last candidate
    assert any(s % 3 == 2 for s in hit) and any(s % 3 == 0 for s in hit) and any(s % 3 == 1 for s in hit)
    assert any(k < 256 for k in cands) and any(256 <= k < 512 for k in cands) and any(k >= 512 for k in cands)
    assert 255 in cands and 256 in cands and 511 in cands and 512 in cands      # both sides of each pass boundary
    assert ch["nrec"][0] == 0 and 0 in [int(d["entry"]) for d in c["records"]]   # entry 0 is not in candidate 0


def test_band_and_time_edges():
    c = _case("band_and_time_edges")
    s = c["channels"][0]["sync"]
    assert {float(r["f1_hz"]) for r in s} >= {K.F1_LO, K.F1_HI} and 10.0 < K.F1_LO < 11.0 and 4989.0 < K.F1_HI < 4990.0
    assert {r["ibest"] for r in s} >= {K.IBEST_LO, K.IBEST_HI} and K.IBEST_LO == -344 - 5 and K.IBEST_HI == 1012 + 5
    assert K.IBEST_HI + 3296 > 4032
    # at the band's lower end the 630-bin window reaches below bin 0: those bins read as +0
    assert int(round(K.F1_LO / (12000.0 / 72576.0))) - 126 < 0


def test_ties_and_near_ties():
    z = _reports(_case("zero_spectrum"))
    assert (z["nsync"] == 4).all() and (z["snr_db"] == -21).all() and not z["xsig"].any() and not z["xnoise"].any()
    assert not np.isnan(z["xsig"]).any()                                # (the restatement's sums are +0 here, not NaN: they are compared on bits)
    words = [d["bits"] for d in _case("zero_spectrum")["records"]]
    G = K.encoder(K.SEED)
    assert [int(r) for r in z["nsymerr"]] == [int((R4.tones(G, w)[list(R4.DATA)] != 0).sum()) for w in words]
    # the carrier halfway between tones 0 and 1: their powers agree to 1 part in 10^4 in every symbol (tone 2 has a ninth of them)
    from oracle import oracle as orc
    import ft4_softbits_ref as S4
    c = _case("half_tone_carrier")
    r = c["channels"][0]["sync"][0]
    zr, zi = S4.symbol_spectra(R4.baseband(orc, K.spectra()["carrier"], r["f1_hz"]).reshape(1, -1), [r["ibest"]])
    P = R4.powers(zr[0], zi[0])
    assert (np.abs(P[:, 0] - P[:, 1]) <= 1e-4 * P[:, 0]).all() and (P[:, 0] > 5 * P[:, 2]).all()


def test_one_huge_term_among_small_ones():
    from oracle import oracle as orc
    import ft4_softbits_ref as S4
    c = _case("huge_and_small")
    assert len({bytes(d["bits"]) for d in c["records"]}) == 1
    t = R4.tones(K.encoder(K.SEED), c["records"][0]["bits"])
    for d, n_huge in zip(c["records"], K.BURST_SYMBOLS):
        r = c["channels"][0]["sync"][int(d["entry"])]
        zr, zi = S4.symbol_spectra(R4.baseband(orc, K.spectra()["burst"], r["f1_hz"]).reshape(1, -1), [r["ibest"]])
        P = R4.powers(zr[0], zi[0]).max(axis=1)
        assert int(np.argmax(P)) == n_huge and P[n_huge] > 50 * np.delete(P, [max(n_huge - 1, 0), n_huge, min(n_huge + 1, 102)]).max(), (n_huge, P[n_huge])
    assert set(K.BURST_SYMBOLS) == {0, 38, 39, 64, 102}                  # lanes 0, 38 (two terms), 39 (one term), and the second terms of lanes 0 and 38


def test_words_of_the_xor_reduction():
    c = _case("xor_reduction")
    G = K.encoder(K.SEED)
    bits = [R4.word_bits(d["bits"]) for d in c["records"]]
    assert any(b.all() for b in bits)                                   # the all-ones word
    single = [int(np.nonzero(b)[0][0]) for b in bits if b.sum() == 1]
    assert {63, 64, 90} <= set(single) and int(np.argmax(G.sum(axis=1))) in single
    assert any(b[64:].all() and not b[:64].any() for b in bits) and any(b[:64].all() and not b[64:].any() for b in bits)


def test_channels():
    c2, c257 = _case("channels_2"), _case("channels_257")
    assert len(c2["channels"]) == 2 and c2["channels"][0]["cnt"] > c2["channels"][0]["cap"] and c2["channels"][1]["cnt"] < c2["channels"][1]["cap"]
    off = c257["offsets"].astype(np.int64)
    counts = np.diff(np.concatenate([off, [len(c257["records"])]]))
    assert len(counts) == 257 and counts[0] == counts[1] == counts[256] == 0 and not counts[100:140].any() and counts[2] == 2 and counts.sum() > 50


def test_the_sent_word():
    r = _reports(_case("sent_word"))
    assert r["nsymerr"][0] == 0 and r["nsync"][0] == 16 and r["snr_db"][0] > 0          # the word that was sent, where it was sent
    assert r["nsymerr"][1] == 0 and r["snr_db"][1] < r["snr_db"][0]                      # one sample early: a little of every symbol is lost
    assert r["nsymerr"][2] > 40 and r["snr_db"][2] == -21                                # two tone spacings off: the signal sits where the noise is taken
    assert r["nsymerr"][3] > 40 and r["nsync"][3] == 16                                  # another word at the right place: the Costas symbols still hit
