"""CPU: the restatement of FT4 a-priori decoding (tests/ft4_ap_ref.py) on hand-made records with the answers written out -- the per-record gate
(BP, OSD, nsync, nqual), the per-set rules (iters = -1, a metric that is not finite), the set-major choice with set = s | p << 2 -- and the
setter's argument errors.  The per-set arithmetic is tests/ap_ref.py's, which tests/test_ap_ref.py holds."""
import os
import re

import numpy as np
import pytest

import ap_cases as C
import ap_ref as AP
import decodes_ref as DR
import ft4_ap_ref as A4
import ft4_decode_cases as D
import ft4_osd_cases as X
import ldpc_cases as LC
import ldpc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
CODE = LC.make_code(C.SEED)["code"]
MIN_NSYNC, MIN_NQUAL = 8, 20
M0, M1 = C.message(7001, C.PREFIXES[0]), C.message(7002, C.PREFIXES[1])        # two words, one under each known field
EMPTY = AP.make_patterns([(np.zeros(0, np.uint8), np.zeros(0, np.uint8))])      # the plain second pass: every clean set is a find under pattern 0
# pattern 0 holds M1's field, pattern 1 holds M0's: a clean set of M0 is contradicted by pattern 0 and found under pattern 1
TWO = AP.make_patterns([C.prefix_pattern(C.PREFIXES[1]), C.prefix_pattern(C.PREFIXES[0])])
NOT_ATTEMPTED = bytes(12) + b"\xff\xff" * 3 + b"\x00\xff" + bytes(4)            # the decode record's "not attempted" bytes, pad_ 0xff, dmin +0


def clean(m91, amp=2.83):
    return (amp * (2.0 * LC.encode(C.SEED, m91) - 1.0)).astype(F32)


def record(sets=(M0, M0, M0), nsync=MIN_NSYNC, nqual=MIN_NQUAL):
    """One record whose three sets hold clean codewords, every set attempted by the decode (iters 30) and failed, OSD attempted and failed."""
    soft = D.soft_dict(np.stack([clean(m) for m in sets])[None], np.ones((1, 3), F32), [nsync], [nqual])
    msg = np.zeros(1, D.MSG4_DTYPE)
    msg["set"]["iters"], msg["set"]["nbad"], msg["set"]["nharderr"] = 30, 9, -1
    osd = np.zeros(1, X.OSD4_DTYPE)
    return soft, msg, osd


def run(soft, msg, osd, patterns=EMPTY):
    return A4.decode(CODE, soft, msg, osd, patterns, C.MAX_ITER, MIN_NSYNC, MIN_NQUAL)[0]


def found(r):
    return [int(x) for x in r["set"]["msg"]["crc_ok"]]


def test_header_and_bindings_state_the_contract_and_keep_the_abi():
    h = open(os.path.join(ROOT, "include", "cwsl_gpu.h")).read()
    assert re.search(r"#define\s+CWSLG_ABI_VERSION\s+5\b", h) and "FT4 a-priori decoding" in h
    import cwsl_digi_amd.api as api
    for name in ("cwslg_set_ft4_ap", "cwslg_fetch_ft4_ap"):
        assert name in h and name in api.ABI_SYMBOLS
    assert not re.search(r"Out of scope:[^/]*FT4 AP", h)
    assert api.ap_set_split(1 | 3 << 2) == (1, 3) and api.ap_set_split(0) == (0, 0) and api.ap_set_split(2 | 7 << 2) == (2, 7)
    s, p = api.ap_set_split(np.array([5, 30], np.uint8))
    assert s.tolist() == [1, 2] and p.tolist() == [1, 7]
    assert A4.split(A4.set_byte(2, 7)) == (2, 7)


def test_a_record_that_passes_the_gate_is_attempted_in_every_set():
    r = run(*record())
    assert found(r) == [1, 1, 1] and [int(x) for x in r["set"]["msg"]["pad_"]] == [0, 0, 0]
    assert all(np.array_equal(R.unpack_bits(r["set"]["msg"]["bits"][s]), M0) for s in range(3))
    assert (r["set"]["msg"]["nharderr"] == 0).all() and (r["set"]["dmin"] == 0).all()      # clean metrics: no disagreeing bit


def test_bp_crc_ok_in_one_set_closes_the_whole_record():
    """BP crc_ok in set 1 alone: nothing is attempted in ANY set -- the gate is per record."""
    soft, msg, osd = record()
    msg["set"]["crc_ok"][0, 1] = 1
    r = run(soft, msg, osd)
    assert all(r["set"][s].tobytes() == NOT_ATTEMPTED for s in range(3))
    assert A4.gate(msg, osd, soft["nsync"], soft["nqual"], MIN_NSYNC, MIN_NQUAL).tolist() == [[False] * 3]


def test_osd_crc_ok_closes_the_record_only_where_the_osd_records_are_used():
    soft, msg, osd = record()
    osd["set"]["crc_ok"][0, 2] = 1
    r = run(soft, msg, osd)
    assert all(r["set"][s].tobytes() == NOT_ATTEMPTED for s in range(3))
    assert found(run(soft, msg, None)) == [1, 1, 1]                       # OSD records not used: attempted


@pytest.mark.parametrize("nsync, nqual, taken", [(MIN_NSYNC, MIN_NQUAL, True), (MIN_NSYNC - 1, MIN_NQUAL, False), (MIN_NSYNC, MIN_NQUAL - 1, False),
                                                 (MIN_NSYNC - 1, 33, False), (16, MIN_NQUAL - 1, False)])
def test_nsync_or_nqual_one_under_the_minimum(nsync, nqual, taken):
    soft, msg, osd = record(nsync=nsync, nqual=nqual)
    r = run(soft, msg, osd)
    assert found(r) == ([1, 1, 1] if taken else [0, 0, 0])
    if not taken:
        assert all(r["set"][s].tobytes() == NOT_ATTEMPTED for s in range(3))


def test_a_set_the_decode_did_not_attempt_is_not_attempted_the_others_are():
    soft, msg, osd = record()
    msg["set"]["iters"][0, 0] = msg["set"]["nbad"][0, 0] = -1           # what the decode writes where sigma[0] == 0
    r = run(soft, msg, osd)
    assert r["set"][0].tobytes() == NOT_ATTEMPTED and found(r) == [0, 1, 1]
    assert A4.best_set(np.array([r]))[0] == 1


def test_a_nan_in_set_1_only():
    soft, msg, osd = record()
    soft["llr"][0, 1, 40] = np.nan
    r = run(soft, msg, osd)
    assert r["set"][1].tobytes() == NOT_ATTEMPTED and found(r) == [1, 0, 1]


def test_the_choice_is_set_major_and_the_set_byte_carries_set_and_pattern():
    """Set 0 holds noise (no find), set 1 a word found under pattern 1, set 2 another word found under pattern 0: the record's word is set 1's,
    though set 2's find came under the earlier pattern, and set = 1 | 1 << 2."""
    soft, msg, osd = record(sets=(M0, M0, M1))
    soft["llr"][0, 0] = (F32(2.83) * np.random.default_rng(8).standard_normal(174)).astype(F32)
    r = run(soft, msg, osd, TWO)
    assert found(r) == [0, 1, 1] and [int(x) for x in r["set"]["msg"]["pad_"]] == [0xff, 1, 0]
    assert r["set"]["msg"]["iters"][0] > 0 and r["set"]["msg"]["nharderr"][0] == -1           # attempted under both patterns, the iterations summed
    assert A4.best_set(np.array([r]))[0] == 1
    where = [(1234.5, 0.25, 3.0)]
    rec, n_total = A4.ap_decodes([(7, where, np.array([r]))])
    assert n_total == 1 and len(rec) == 1
    d = rec[0]
    assert (int(d["ch_id"]), int(d["entry"]), int(d["by_osd"]), int(d["set"]), int(d["ndup"])) == (7, 0, 2, 1 | 1 << 2, 1)
    assert d["bits"].tobytes() == C.bits12(M0) and A4.split(d["set"]) == (1, 1)
    assert d["dmin"] == r["set"]["dmin"][1] and d["nharderr"] == r["set"]["msg"]["nharderr"][1]
    assert (np.float32(d["freq_hz"]), np.float32(d["dt_s"]), np.float32(d["sync"])) == tuple(np.float32(v) for v in where[0])


def test_equal_words_of_two_entries_fold_and_the_zero_word_is_dropped():
    a = np.zeros(3, A4.AP4_DTYPE)
    a["set"]["msg"]["pad_"] = 0xff
    for q, (s, p, nh) in enumerate([(2, 3, 9), (0, 1, 4)]):
        a["set"]["msg"][q, s] = (np.frombuffer(C.bits12(M0), np.uint8), 5, 0, nh, 1, p)
        a["set"]["dmin"][q, s] = 1.5 + q
    a["set"]["msg"][2, 0] = (np.zeros(12, np.uint8), 0, 0, 0, 1, 0)     # the all-zero word under an all-zero pattern: no decode
    rec, n_total = A4.ap_decodes([(3, [(100.0 * q, 0.1, 2.0) for q in range(3)], a)])
    assert n_total == 1 and (int(rec[0]["entry"]), int(rec[0]["set"]), int(rec[0]["ndup"]), int(rec[0]["nharderr"])) == (1, 0 | 1 << 2, 2, 4)
    assert rec[0]["dmin"] == F32(2.5) and rec.dtype == DR.DECODE_DTYPE


def test_the_setters_errors():
    ok = C.patterns(2)
    assert A4.validate(ok) == 0 and A4.validate(ok[:0]) == 0 and A4.validate(C.patterns(8)) == 0
    assert A4.validate(ok, max_iter=0) == 4 and A4.validate(ok, max_iter=201) == 4 and A4.validate(ok, max_iter=200) == 0
    assert A4.validate(ok, min_nsync=-1) == 4 and A4.validate(ok, min_nsync=18) == 4 and A4.validate(ok, min_nsync=17) == 0
    assert A4.validate(ok, min_nqual=-1) == 4 and A4.validate(ok, min_nqual=34) == 4 and A4.validate(ok, min_nqual=33) == 0
    assert A4.validate(ok, n_pat=9) == 1 and A4.validate(ok, n_pat=-1) == 1
    bad = ok.copy()
    bad["mask"][1, 11] |= 0x10                                           # position 91
    assert A4.validate(bad) == 2
    bad = ok.copy()
    bad["mask"][0, 0] &= 0x7f
    bad["value"][0, 0] |= 0x80                                           # a value bit outside its mask
    assert A4.validate(bad) == 3
    # 17 and 33 are in range and mean that nothing is attempted: no record has nsync 17 or nqual 33
    soft, msg, osd = record(nsync=16, nqual=32)
    assert not A4.gate(msg, osd, soft["nsync"], soft["nqual"], 17, 0).any() and not A4.gate(msg, osd, soft["nsync"], soft["nqual"], 0, 33).any()
