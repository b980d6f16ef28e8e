"""CPU: the restatement of FT8 a-priori decoding (tests/ap_ref.py) on hand-made metric sets with the answers written out -- one case per rule of
the contract in include/cwsl_gpu.h -- the setter's argument errors, and the host header (csrc/ap_host.hpp) against the restatement through a
stand-alone program, plain and under -fsanitize=address,undefined."""
import os
import re
import subprocess

import numpy as np
import pytest

import ap_cases as C
import ap_ref as AP
import ldpc_cases as LC
import ldpc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CODE = LC.make_code(C.SEED)["code"]


def run(name):
    pat, x, word = C.rule_cases()[name]
    return AP.decode(CODE, x[None], pat, C.MAX_ITER)[0], pat, x, word


def fields(r):
    m = r["msg"]
    return (int(m["iters"]), int(m["nbad"]), int(m["nharderr"]), int(m["crc_ok"]), int(m["pad_"]), float(r["dmin"]))


def test_header_states_the_contract_and_keeps_the_abi():
    h = open(os.path.join(ROOT, "include", "cwsl_gpu.h")).read()
    assert re.search(r"#define\s+CWSLG_ABI_VERSION\s+5\b", h)                  # exports were added, nothing else changed
    for name in ("cwslg_set_ft8_ap", "cwslg_fetch_ft8_ap", "cwslg_ap_decode", "cwslg_ap_pattern", "cwslg_ap_msg"):
        assert name in h
    import cwsl_digi_amd.api as api
    for name in ("cwslg_set_ft8_ap", "cwslg_fetch_ft8_ap", "cwslg_ap_decode"):
        assert name in api.ABI_SYMBOLS
    assert api.AP_MSG_DTYPE == AP.AP_MSG_DTYPE and api.AP_PATTERN_DTYPE == AP.PATTERN_DTYPE


@pytest.mark.parametrize("name", ["nan", "inf"])
def test_a_metric_that_is_not_finite_is_not_attempted(name):
    r, *_ = run(name)
    assert fields(r) == (-1, -1, -1, 0, 0xff, 0.0) and not r["msg"]["bits"].any()
    assert r.tobytes() == bytes(12) + b"\xff\xff" * 3 + b"\x00\xff" + bytes(4)


def test_all_zero_metrics():
    """A = 0: the forced metrics are +-0 and z > 0 is false everywhere, so the loop leaves at once with the all-zero word.  Under a pattern whose
    value has a one it contradicts the pattern; under an all-zero value it is the find (which the fetch then drops as the all-zero word)."""
    r, pat, x, _ = run("zeros")
    assert np.unpackbits(pat["value"][0]).any()
    assert fields(r) == (0, 0, -1, 0, 0xff, 0.0) and not r["msg"]["bits"].any()
    r, *_ = run("zeros_zero_value")
    assert fields(r) == (0, 0, 0, 1, 0, 0.0) and not r["msg"]["bits"].any()


@pytest.mark.parametrize("name", ["empty_mask_clean", "empty_mask_noise"])
def test_an_empty_mask_is_the_decode_contract(name):
    """The two texts of the loop agree: under an empty mask the record is ldpc_ref.decode's on the same metrics."""
    r, pat, x, word = run(name)
    want = R.decode(CODE, x[None], C.MAX_ITER)[0]
    cw, iters, nbad = AP.bp(CODE, x[None], C.MAX_ITER)
    assert (iters[0], nbad[0]) == (want["iters"], want["nbad"]) and np.array_equal(R.pack_bits(cw[0]), want["bits"])
    assert int(((x > 0) != cw[0]).sum()) == want["nharderr"]
    if name == "empty_mask_clean":
        assert want["crc_ok"] == 1 and fields(r) == (1, 0, 1, 1, 0, float(r["dmin"]))
        assert r["msg"].tobytes()[:19] == want.tobytes()[:19] and np.array_equal(R.unpack_bits(r["msg"]["bits"]), word)
        assert r["dmin"] == AP.distance(x, cw[0]) and r["dmin"] > 0
    else:
        assert want["crc_ok"] == 0 and fields(r) == (12, 23, -1, 0, 0xff, 0.0) and (want["iters"], want["nbad"]) == (12, 23)


def test_all_77_bits_masked():
    r, pat, x, word = run("all77")
    assert np.unpackbits(pat["mask"][0]).sum() == 77 and R.decode(CODE, x[None], C.MAX_ITER)[0]["crc_ok"] == 0
    assert fields(r)[:5] == (7, 0, 33, 1, 0) and np.array_equal(R.unpack_bits(r["msg"]["bits"]), word)


def test_first_pattern_wrong_second_right():
    """pad_ = 1 and iters is that run's alone (the first run went to max_iter)."""
    r, pat, x, word = run("second_right")
    first = AP.decode(CODE, x[None], pat[:1], C.MAX_ITER)[0]
    assert fields(first) == (30, 17, -1, 0, 0xff, 0.0)
    assert fields(r)[:5] == (8, 0, 21, 1, 1) and np.array_equal(R.unpack_bits(r["msg"]["bits"]), word)
    assert r["dmin"] == AP.distance(x, LC.encode(C.SEED, word).astype(bool))


def test_no_success_sums_the_iterations():
    r, pat, x, _ = run("no_success")
    assert len(pat) == 3 and fields(r) == (90, 14, -1, 0, 0xff, 0.0) and not r["msg"]["bits"].any()
    assert [int(AP.decode(CODE, x[None], pat[p:p + 1], C.MAX_ITER)[0]["msg"]["iters"]) for p in range(3)] == [30, 30, 30]


def test_dmin_and_nharderr_are_taken_on_the_original_metrics():
    """Bit 3 is told to the decoder and the channel contradicts it with |llr| = 5: the word found differs from the ORIGINAL hard decisions there
    and nowhere else, so nharderr = 1 and dmin = 5 -- against the modified metrics both would be 0."""
    r, pat, x, word = run("original_metrics")
    assert (x[3] > 0) != bool(word[3]) and abs(float(x[3])) == 5.0
    assert fields(r) == (0, 0, 1, 1, 0, 5.0) and np.array_equal(R.unpack_bits(r["msg"]["bits"]), word)


def test_a_word_that_contradicts_its_pattern_is_no_find():
    """Under the REAL loop: metrics of +-10 for a codeword, a pattern that differs from it in bit 5.  One iteration turns the forced bit back: the
    loop leaves with the codeword (nbad 0, CRC right), which disagrees with the pattern -- no success."""
    r, pat, x, word = run("contradicts")
    mask, value = np.unpackbits(pat["mask"][0])[:R.K].astype(bool), np.unpackbits(pat["value"][0])[:R.K].astype(bool)
    A = F32(1.01) * np.abs(x).max()
    lp = x.copy()
    lp[:R.K] = np.where(mask, np.where(value, A, -A), lp[:R.K])
    cw, iters, nbad = AP.bp(CODE, lp[None], C.MAX_ITER)
    assert (iters[0], nbad[0]) == (1, 0) and np.array_equal(cw[0][:R.K], word.astype(bool))
    assert R.crc14(cw[0][:77]) == R.crc_field(cw[0][:R.K])
    assert np.nonzero(cw[0][:R.K][mask] != value[mask])[0].tolist() == [5]
    assert fields(r) == (1, 0, -1, 0, 0xff, 0.0) and not r["msg"]["bits"].any()


def test_the_setters_argument_errors():
    ok = C.patterns(8)
    assert AP.validate(ok) == 0 and AP.validate(ok[:0]) == 0
    assert AP.validate(np.zeros(9, AP.PATTERN_DTYPE)) == 1 and AP.validate(ok, n_pat=-1) == 1
    for t in range(91, 96):
        bad = ok.copy()
        bad["mask"][2][t >> 3] |= 0x80 >> (t & 7)
        assert AP.validate(bad) == 2
    bad = ok.copy()
    bad["value"][7][11] |= 0x01                                             # position 95, value alone: the position rule comes first
    assert AP.validate(bad) == 2
    bad = ok.copy()
    bad["value"][5][4] |= 0x10                                              # pattern 5 has an empty mask
    assert AP.validate(bad) == 3
    assert AP.validate(AP.make_patterns([(np.zeros(0), np.zeros(0))])) == 0  # a mask with no bit set is allowed
    for it, ns in ((0, 7), (201, 7), (30, -1), (30, 23)):
        assert AP.validate(ok, max_iter=it, min_nsync=ns) == 4
    assert AP.validate(ok, max_iter=1, min_nsync=0) == 0 and AP.validate(ok, max_iter=200, min_nsync=22) == 0


# ---- the host header against the restatement ----------------------------------------------------------------------------------------------------
def _pattern_sets():
    ok = C.patterns(8)
    sets = [(n, ok[:n]) for n in (0, 1, 2, 8)] + [(9, ok), (-1, ok[:0]), (3, ok[:0])]
    rng = np.random.default_rng(12)
    for _ in range(40):                                                     # random bytes: most break a rule somewhere
        n = int(rng.integers(1, 9))
        p = np.zeros(n, AP.PATTERN_DTYPE)
        p["mask"] = rng.integers(0, 256, (n, 12))
        p["value"] = p["mask"] & rng.integers(0, 256, (n, 12))
        kind = rng.integers(0, 4)
        if kind >= 1:
            p["mask"][:, 11] &= 0xe0
            p["value"][:, 11] &= 0xe0
        if kind == 2:
            p["value"][n - 1][int(rng.integers(0, 11))] |= 0x04
        sets.append((n, p))
    return sets


@pytest.mark.parametrize("sanitize", [False, True])
def test_host_header_matches_the_restatement(tmp_path, sanitize):
    exe = str(tmp_path / "ap_host_check")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [os.path.join(ROOT, "tests", "ap_host_check.cpp"), "-o", exe])
    sets = _pattern_sets()
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.uint32(len(sets)).tobytes())
        for n, p in sets:
            fh.write(np.int32(n).tobytes() + np.uint32(len(p)).tobytes() + p.tobytes())
    subprocess.check_call([exe, fin, fout])
    got = np.frombuffer(open(fout, "rb").read(), np.dtype([("why", np.int32), ("block", np.uint32, (8, 6))]))
    assert len(got) == len(sets)
    seen = set()
    for (n, p), g in zip(sets, got):
        want = 1 if (n > 0 and len(p) == 0) else AP.validate(p, n_pat=n)
        assert g["why"] == want
        seen.add(want)
        if want == 0:
            assert np.array_equal(g["block"], AP.pack_block(p[:n]))
        else:
            assert (g["block"] == 0xEEEEEEEE).all()                         # a rejected set leaves the block alone
    assert seen == {0, 1, 2, 3}
