"""CPU: the cases of tests/report_kernel_cases.py contain what tests/test_gpu_report_kernel.py needs them to contain -- proved with
tests/decode_reports_ref.py alone -- and the case file is what tests/report_kernel_check.hip reads."""
import os
import struct

import numpy as np

import decode_reports_ref as RR
import report_kernel_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BY_NAME = {c["name"]: c for c in K.cases()}


def _reports(case):
    n = min(case["n_total"], case["lim"])
    return K.answer(case)[:K.REP_WORDS * n].view(RR.REPORT_DTYPE)


def test_decode_counts_cover_every_wave_position():
    assert [len(BY_NAME[f"decodes_{n}"]["records"]) for n in (1, 3, 4, 5, 63, 64, 65)] == [1, 3, 4, 5, 63, 64, 65]


def test_edges():
    for pitch in (32, 992):
        case = BY_NAME[f"edges_pitch_{pitch}"]
        ch = case["channels"][0]
        assert ch["plane"].shape == (RR.NHSYM, pitch)
        ij = [(int(c["freq_bin"]), int(c["time_step"])) for c in ch["list"]]
        assert (0, -62) in ij and (0, 62) in ij and (pitch - 15, 62) in ij and (pitch - 15, -62) in ij
        assert (pitch - 15) + 14 == pitch - 1                           # tone 7 of that position is the row's last bin
        assert any(i + 14 >= pitch for i, _ in ij)                      # and positions whose upper tones lie beyond the row
        used = {int(r["entry"]) for r in case["records"]}
        assert used == set(range(len(ij)))
        # j = -62: symbols 0..12 lie before step 1; j = +62: symbols 75..78 after step 372
        assert not RR.plane_powers(ch["plane"], 0, -62)[:13].any() and RR.plane_powers(ch["plane"], 0, -62)[13].all()
        assert not RR.plane_powers(ch["plane"], 0, 62)[75:].any() and RR.plane_powers(ch["plane"], 0, 62)[74].all()


def test_equal_plane_puts_every_maximum_at_tone_0():
    case = BY_NAME["equal_plane"]
    G = K.encoder(case["seed"])
    rep = _reports(case)
    for r, d in zip(rep, case["records"]):
        t = RR.tones(G, d["bits"])
        j = int(case["channels"][0]["list"][int(d["entry"])]["time_step"])
        inside = np.array([1 <= j + 12 + 4 * n <= RR.NHSYM for n in range(RR.NSYM)])
        # (a symbol outside the plane is all +0: its first maximum is at tone 0 as well)
        assert r["nsync"] == 3 and r["nsymerr"] == int((t[list(RR.DATA)] != 0).sum()) and inside.sum() in (79, 66)
    assert len({int(r["nsymerr"]) for r in rep}) > 1


def test_huge_and_tiny_depends_on_the_order():
    case = BY_NAME["huge_and_tiny"]
    G = K.encoder(case["seed"])
    differs = 0
    for ch, d in zip(case["channels"], case["records"]):
        t = RR.tones(G, d["bits"]).astype(int)
        P = RR.plane_powers(ch["plane"], 2, 3)
        terms = P[np.arange(79), t]
        assert (terms > 1e7).sum() == 1 and (terms < 1).sum() == 78
        seq = np.float32(0)
        for v in terms:
            seq = np.float32(seq + v)
        differs += RR.tree79(terms) != seq
    assert differs >= 1                                                 # the sequential sum is not the tree's: the order is observable


def test_xor_reduction_words():
    case = BY_NAME["xor_reduction"]
    G = K.encoder(case["seed"])
    bits = [RR.word_bits(d["bits"]) for d in case["records"]]
    assert any(b.all() for b in bits)                                   # the all-ones word
    singles = [int(np.nonzero(b)[0][0]) for b in bits if b.sum() == 1]
    assert {63, 64, 90} <= set(singles) and int(np.argmax(G.sum(axis=1))) in singles
    assert any(b[64:].all() and not b[:64].any() for b in bits) and any(b[:64].all() and not b[64:].any() for b in bits)


def test_channel_layouts():
    assert len(BY_NAME["channels_2"]["channels"]) == 2 and len(BY_NAME["decodes_1"]["channels"]) == 1
    case = BY_NAME["channels_257"]
    off = case["offsets"].astype(int)
    counts = np.diff(np.append(off, len(case["records"])))
    assert len(off) == 257 and counts[0] == 0 and counts[1] == 0 and counts[256] == 0 and not counts[100:140].any() and counts.sum() > 100
    assert counts[2] > 0 and counts[255] > 0


def test_limits():
    a, b = BY_NAME["limit_below_total"], BY_NAME["limit_above_total"]
    assert a["lim"] < a["n_total"] and b["lim"] > b["n_total"]
    assert (K.answer(a)[K.REP_WORDS * a["lim"]:] == K.AB).all()


def test_case_file_is_what_the_program_reads(tmp_path):
    cs = K.cases()[:2]
    path = str(tmp_path / "cases.bin")
    K.write_cases(path, cs)
    raw = open(path, "rb").read()
    assert raw[:4] == b"RPK1" and struct.unpack_from("<i", raw, 4)[0] == 2
    n_chan, n_total, lim = struct.unpack_from("<3i", raw, 8)
    assert (n_chan, n_total, lim) == (1, 1, 1)
    at = 20 + 546 * 4 + 4 * n_chan
    nbins, cap = struct.unpack_from("<2i", raw, at)
    assert (nbins, cap) == (32, 16)
    src = open(os.path.join(ROOT, "tests", "report_kernel_check.hip")).read()
    assert "report_launch(" in src and "hipLaunchKernelGGL" not in src   # the launch is the library's
    host = open(os.path.join(ROOT, "cwsl_digi_amd", "csrc", "sync_host.inc")).read()
    assert "report_launch(" in host
