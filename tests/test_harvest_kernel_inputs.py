"""CPU: the cases of tests/harvest_kernel_cases.py contain what tests/test_gpu_harvest_kernel.py needs them to contain -- every carry of
decode_harvest_kernel between two passes, every poisoned place -- proved with tests/decodes_ref.py alone; the hand-written answers equal
decodes_ref's; and the check program compiles for gfx950 (it is not run here).  If a property is missing the seeds or the builders change, not
the assertions."""
import os

import numpy as np

import decodes_ref as DR
import harvest_kernel_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NT = K.NT


def _carriers(case, ch):
    """word -> [(entry, by_osd, nharderr, set)] of one channel, before de-duplication; and the number of entries."""
    _, where, msg, osd = K.channel_input(case, ch)
    out = {}
    for q in range(len(msg)):
        w = (DR._word_ft4 if case["ft4"] else DR._word_ft8)(msg[q], None if osd is None else osd[q])
        if w is not None and not DR.all_zero_word(w[2]):
            out.setdefault(w[2], []).append((q, w[0], w[3], w[1]))
    return out, len(msg)


def _one(name, i=0):
    case = K.family(name)[i]
    recs, counts = K.answer(case)
    return case, case["channels"][0], recs, counts


def _same_records(recs, literal):
    assert len(recs) == len(literal) and recs.tobytes() == (np.array(literal, DR.DECODE_DTYPE).tobytes() if literal else b""), (recs, literal)


def test_every_case_has_a_name_of_its_own_and_arrays_of_its_cap():
    cases = [c for _, _, c in K.all_cases()]
    assert len({c["name"] for c in cases}) == len(cases)
    for c in cases:
        assert c["max_out"] >= 0 and len(c["channels"]) >= 1
        for ch in c["channels"]:
            assert 1 <= ch["cap"] <= K.MAXCAND and len(ch["list"]) == len(ch["msg"]) == len(ch["osd"]) == ch["cap"]


def test_ft8_distinct_words_at_every_count():
    """cnt 0, -1, 1, 255, 256, 257, 600 and 700 at cap 600 and 9 at cap 5: slots = words = survivors = min(cnt, cap), all by BP, and the entries
    from the count on carry words too."""
    assert [(c["channels"][0]["cap"], c["channels"][0]["cnt"]) for c in K.family("ft8_distinct")] == \
        [(600, 0), (600, -1), (600, 1), (600, 255), (600, 256), (600, 257), (600, 600), (600, 700), (5, 9)]
    for i in range(len(K.FT8_COUNTS)):
        case, ch, recs, counts = _one("ft8_distinct", i)
        n = max(0, min(ch["cnt"], ch["cap"]))
        assert len(recs) == n and list(recs["entry"]) == list(range(n)) and not recs["by_osd"].any() and (recs["ndup"] == 1).all()
        assert ch["msg"]["crc_ok"].all() and len({bytes(b) for b in ch["msg"]["bits"]}) == ch["cap"]


def test_ft8_crowded_channel_passes_256_three_times():
    case, ch, recs, _ = _one("ft8_crowded")
    car, n = _carriers(case, ch)
    listed = sum(len(v) for v in car.values())
    assert n == 600 and listed > NT and len(recs) > NT, (listed, len(recs))
    assert recs["by_osd"].any() and not recs["by_osd"].all() and recs["ndup"].max() >= 3
    assert 0.45 < ch["msg"]["crc_ok"].mean() < 0.55 and 0.35 < ch["osd"]["crc_ok"].mean() < 0.45
    # a winner that is not the smallest entry carrying its word, and one that wins on nharderr among BP entries
    late = [r for r in recs if int(r["entry"]) != min(q for q, *_ in car[bytes(r["bits"])])]
    assert late and any(not r["by_osd"] and sum(1 for _, by, *_ in car[bytes(r["bits"])] if not by) >= 2 for r in late)
    # the same records without OSD: other bytes, BP only
    case0, ch0, recs0, _ = _one("ft8_crowded", 1)
    assert ch0["osd_null"] and not ch["osd_null"] and ch0["msg"].tobytes() == ch["msg"].tobytes() and ch0["osd"].tobytes() == ch["osd"].tobytes()
    assert 0 < len(recs0) < len(recs) and not recs0["by_osd"].any()


def test_ft8_one_word():
    for i, (entry, nharderr) in enumerate(((599, 80), (300, 2))):
        case, ch, recs, _ = _one("ft8_one_word", i)
        car, n = _carriers(case, ch)
        assert n == 600 and len(car) == 1 and len(recs) == 1
        assert (int(recs[0]["entry"]), int(recs[0]["by_osd"]), int(recs[0]["nharderr"]), int(recs[0]["ndup"])) == (entry, 0, nharderr, 600)
        _same_records(recs, case["literal"])
    ch = K.family("ft8_one_word")[0]["channels"][0]
    assert ch["msg"]["crc_ok"].sum() == 1 and ch["msg"]["crc_ok"][599] and ch["osd"]["crc_ok"][:599].all()
    ch = K.family("ft8_one_word")[1]["channels"][0]
    nh = ch["msg"]["nharderr"]
    assert ch["msg"]["crc_ok"].all() and nh[300] == nh[511] == nh.min() and (nh == nh.min()).sum() == 2


def test_ft8_rank_across_passes():
    case, ch, recs, _ = _one("ft8_rank_across_passes")
    car, _ = _carriers(case, ch)
    assert sorted(v for v in car.values() if len(v) == 3) == [[(0, 1, 0, 0), (2, 0, 9, 0), (580, 0, 3, 0)]]
    assert list(recs["entry"]) == [1, 100, 300, 579, 580, 581, 599] and list(recs["ndup"]) == [1, 1, 1, 1, 3, 1, 1]
    assert 580 // NT != 2 // NT                                         # the winner and the BP entry it beats are listed in different passes
    _same_records(recs, case["literal"])


def test_ft8_keys():
    case, ch, recs, _ = _one("ft8_keys", 0)
    words = [np.frombuffer(bytes(r["bits"]), "<u4") for r in recs]
    diff = [tuple(int(x) for x in words[0] ^ w) for w in words[1:]]
    assert [sum(bin(x).count("1") for x in d) for d in diff] == [1, 1, 1, 1]                  # one bit each
    assert [tuple(bool(x) for x in d) for d in diff] == [(True, False, False), (False, True, False), (False, False, True), (False, False, True)]
    assert recs[3]["bits"][11] ^ recs[0]["bits"][11] == 0x20 and recs[4]["bits"][11] ^ recs[0]["bits"][11] == 0x01
    assert list(recs["entry"]) == [0, 1, 2, 3, 5] and list(recs["ndup"]) == [2, 1, 1, 1, 1] and ch["cnt"] == 6 and ch["msg"]["crc_ok"][6:].all()
    _same_records(recs, case["literal"])
    case, ch, recs, _ = _one("ft8_keys", 1)
    m, o = ch["msg"], ch["osd"]
    assert m["crc_ok"][0] and bytes(m["bits"][0]) == bytes(11) + b"\x1f" and not o["crc_ok"][0]                   # zero word, padding set, by BP
    assert not m["crc_ok"][1] and o["crc_ok"][1] and bytes(o["bits"][1]) == bytes(11) + b"\x1f"                   # ... by OSD
    assert m["crc_ok"][2] and not m["bits"][2].any() and o["crc_ok"][2] and o["bits"][2].any()                    # zero BP word over a good OSD word
    assert not m["crc_ok"][3] and m["pad_"][3] == 0xFF and not o["crc_ok"][3] and o["how"][3] and o["flip"][3].all()
    assert m["crc_ok"][4] == 0x80 and o["crc_ok"][5] == 0x80
    assert [(int(r["entry"]), int(r["by_osd"]), int(r["ndup"])) for r in recs] == [(5, 1, 1), (6, 0, 2)]
    _same_records(recs, case["literal"])


def test_ft4_crowded_channel():
    case, ch, recs, _ = _one("ft4_crowded")
    car, n_entries = _carriers(case, ch)
    nrec = ch["nrec"]
    assert n_entries == nrec.sum() > NT and sum(len(v) for v in car.values()) > NT and len(recs) > NT
    assert set(nrec) == {0, 1, 2, 3} and (nrec[K.FT4_RUN[0]:K.FT4_RUN[1]] == 0).all() and K.FT4_RUN[1] - K.FT4_RUN[0] >= 100
    exists = np.arange(3)[None, :] < nrec[:, None]
    assert any(not exists.reshape(-1)[b:b + NT].any() for b in range(0, 1800, NT))            # a whole pass without an existing slot
    assert exists.reshape(-1)[1800 - 1800 % NT:].any()                                       # and entries after it
    bp, osd = ch["msg"]["set"]["crc_ok"] != 0, ch["osd"]["set"]["crc_ok"] != 0
    assert bp[~exists].any(axis=-1).all() and osd[~exists].any(axis=-1).all()                # every slot that does not exist is poisoned
    assert 0.2 < bp[exists].mean() < 0.3 and 0.25 < osd[exists].mean() < 0.35
    for by in (0, 1):
        assert set(recs["set"][recs["by_osd"] == by]) == {0, 1, 2}
    assert (bp[exists][:, 2] & ~bp[exists][:, 0] & ~bp[exists][:, 1] & osd[exists][:, 0]).any()                   # BP of set 2 over an OSD of set 0
    d = ch["osd"]["set"]["dmin"]
    assert (d[..., 0] != d[..., 1]).all() and (d[..., 1] != d[..., 2]).all() and (d[..., 0] != d[..., 2]).all()
    assert (ch["list"]["f0_hz"] != ch["list"]["f1_hz"]).all()
    assert recs["ndup"].max() >= 3 and any(int(r["entry"]) != min(q for q, *_ in car[bytes(r["bits"])]) for r in recs)
    # ignoring nrec, or taking the slot for the entry, gives another answer
    blind = dict(ch, nrec=np.full(600, 3, np.int32))
    assert K.answer(dict(case, channels=[blind]))[0].tobytes() != recs.tobytes()
    case0, ch0, recs0, _ = _one("ft4_crowded", 1)
    assert ch0["osd_null"] and ch0["msg"].tobytes() == ch["msg"].tobytes() and NT < len(recs0) < len(recs) and not recs0["by_osd"].any()


def test_ft4_small():
    for i, nrec in enumerate((0, 1, 3)):
        case, ch, recs, _ = _one("ft4_small", i)
        assert (ch["cap"], ch["cnt"], list(ch["nrec"])) == (2, 1, [nrec, 3]) and (ch["msg"]["set"]["crc_ok"][:, :, 1] != 0).all()
        assert list(recs["entry"]) == list(range(nrec)) and (recs["set"] == 1).all() and not recs["by_osd"].any()
        _same_records(recs, case["literal"])
    case, ch, recs, _ = _one("ft4_small", 3)
    assert (ch["cnt"], list(ch["nrec"])) == (86, [3] * 86) and 3 * 86 == NT + 2
    assert [(int(r["entry"]), int(r["by_osd"]), int(r["set"]), int(r["ndup"])) for r in recs] == [(0, 0, 1, 1), (255, 1, 2, 1), (256, 0, 2, 1), (257, 0, 0, 2)]
    _same_records(recs, case["literal"])


def test_many_channels_feed_the_scan():
    """1, 255, 256, 257 and 600 channels: ch_id = 3 i + 1, counts of 0..4; from 255 channels on every aligned stretch of 64 channels (a wave of the
    scan) has decodes and there are 64 channels in a row without any; equal words in two channels are two decodes."""
    assert [len(c["channels"]) for c in K.family("ft8_channels")] == [1, 255, 256, 257, 600]
    pools = set()
    for case, (c, o, out) in zip(K.family("ft8_channels"), K.expected("ft8_channels")):
        chans, n = case["channels"], len(case["channels"])
        recs, counts = K.answer(case)
        assert [ch["ch_id"] for ch in chans] == [3 * i + 1 for i in range(n)] and all(ch["cap"] == 4 and 0 <= ch["cnt"] <= 4 for ch in chans)
        assert list(c[:n]) == counts and list(o[:n]) == [sum(counts[:i]) for i in range(n)] and (c[n:] == K.AB).all() and (o[n:] == K.AB).all()
        assert out[0] == sum(counts) and max(counts) <= 4
        pools |= {bytes(b) for b in recs["bits"]}
        if n < 255:
            continue
        assert {ch["cnt"] for ch in chans} == {0, 1, 2, 3, 4} and max(counts) >= 3
        assert all(any(counts[b:b + 64]) for b in range(0, n, 64)), [sum(counts[b:b + 64]) for b in range(0, n, 64)]
        assert any(not any(counts[b:b + 64]) for b in range(n - 63))
        assert all(any(counts[b:b + NT]) for b in range(0, n, NT))                          # every pass adds to the carry
        by_word = {}
        for r in recs:
            by_word.setdefault(bytes(r["bits"]), set()).add(int(r["ch_id"]))
        assert max(len(v) for v in by_word.values()) >= 2
        assert recs["ndup"].max() >= 2 and recs["by_osd"].any() and not recs["by_osd"].all()
    assert len(pools) == 8


def test_truncation_cases():
    cases = K.family("truncation")
    for name, base in (("ft8_channels_600", K.family("ft8_channels")[4]), ("ft8_crowded", K.family("ft8_crowded")[0])):
        recs, counts = K.answer(base)
        total = len(recs)
        assert total > NT + 2
        mine = [c for c in cases if c["name"].startswith(name + "_max")]
        assert all(c["channels"] == base["channels"] for c in mine)
        cuts = [c["max_out"] for c in mine]
        assert cuts[:8] == [0, 1, 255, 256, 257, total - 1, total, total + 8] and len(cuts) == 9
        offs = np.concatenate([[0], np.cumsum(counts)])
        assert any(offs[i] < cuts[8] < offs[i + 1] for i in range(len(counts))), cuts[8]      # cuts inside a channel
    for case, (c, o, out) in zip(cases, K.expected("truncation")):
        n = min(int(out[0]), case["max_out"])
        assert (out[K.HEAD_WORDS + K.REC_WORDS * n:] == K.AB).all() and len(out) == K.HEAD_WORDS + K.REC_WORDS * (case["max_out"] + 8)
        assert n == 0 or (out[K.HEAD_WORDS:K.HEAD_WORDS + K.REC_WORDS * n] != K.AB).any()


def test_case_file_round_trip(tmp_path):
    """write_cases writes what harvest_kernel_check.hip reads: header words, then arrays of the sizes its comment states; read_results reads what
    blocks() lays out."""
    cases = [c for _, _, c in K.all_cases()]
    path = tmp_path / "cases.bin"
    K.write_cases(path, cases)
    per = lambda c, ch: 16 + ch["cap"] * ((96 + 4 + 180 + 216) if c["ft4"] else (20 + 20 + 24))
    assert os.path.getsize(path) == 8 + sum(12 + sum(per(c, ch) for ch in c["channels"]) for c in cases)
    want = [b for name in K.FAMILIES for b in K.expected(name)]
    words = [np.array([int.from_bytes(b"HVR1", "little"), len(cases)], np.uint32)]
    for c, (cn, of, out) in zip(cases, want):
        words += [np.array([len(c["channels"]), c["max_out"]], np.uint32), cn, of, out]
    np.concatenate(words).tofile(tmp_path / "res.bin")
    got = K.read_results(tmp_path / "res.bin", cases)
    assert all(K.first_difference(c, g, w) == "" for c, g, w in zip(cases, got, want))
    bad = [a.copy() for a in got[3]]
    bad[2][K.HEAD_WORDS + 12] ^= 1
    assert "record 1 of" in K.first_difference(cases[3], bad, want[3]) and cases[3]["name"] in K.first_difference(cases[3], bad, want[3])


def test_check_program_compiles_for_gfx950(tmp_path):
    exe = K.build_check_program(tmp_path)
    assert os.path.getsize(exe) > 0
    src = open(os.path.join(ROOT, "tests", "harvest_kernel_check.hip")).read()
    assert "harvest_launch(" in src and "hipLaunchKernelGGL" not in src                       # the launches are the library's
    host = open(os.path.join(ROOT, "cwsl_digi_amd", "csrc", "sync_host.inc")).read()
    assert "harvest_launch(" in host and "decode_harvest_kernel," not in host
