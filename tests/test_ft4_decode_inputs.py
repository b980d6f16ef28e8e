"""CPU: the inputs of tests/test_gpu_ft4_decode.py, checked before any GPU sees them -- the recipes of tests/ft4_decode_cases.py on the CPU oracle's
own records (oracle.ft4_sync_all + ft4_softbits_ref.softbits_of_records) with the restatement alone -- and the FT4 decode's surface: header,
ABI version, record size in C, ctypes and numpy, exports, shim.  If a property is missing the recipes change, not these assertions."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import ft4_decode_cases as D
import ft4_softbits_ref as S
import ldpc_cases as C
import ldpc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tones_invert_tone_bits():
    rng = np.random.default_rng(5)
    for _ in range(4):
        cw = rng.integers(0, 2, 174)
        t = D.tones_of(cw)
        assert t.shape == (103,) and t.min() >= 0 and t.max() <= 3 and np.array_equal(S.tone_bits(t), cw)
        assert [list(t[b:b + 4]) for b in (0, 33, 66, 99)] == [list(r) for r in D.ICOS4]


def test_expected_applies_the_restatement_per_set_with_both_gates():
    seed = C.SEEDS[0]
    code = C.make_code(seed)["code"]
    llr = C.metric_sets(seed)[0]
    soft = D.soft_dict(np.stack([llr[[0, 2, 8]]] * 4), [[1, 1, 0], [1, 1, 1], [1, 1, 1], [0, 0, 0]], [8, 7, 8, 16], [20, 20, 19, 32])
    e = D.expected(soft, code, 30, 8, 20)
    ref = C.reference_records(seed, 30)
    assert e.dtype.itemsize == 60 and e["set"].shape == (4, 3)
    assert e["set"][0, 0] == ref[0] and e["set"][0, 1] == ref[2]
    na = np.zeros(1, R.MSG_DTYPE)[0]
    na["iters"] = na["nbad"] = na["nharderr"] = -1
    assert e["set"][0, 2] == na                                         # sigma[2] == 0: that set alone
    assert all(e["set"][q, s] == na for q in (1, 2, 3) for s in range(3))   # nsync 7 < 8; nqual 19 < 20; every sigma 0
    assert D.best_set(e).tolist() == [0, -1, -1, -1]
    assert len(D.expected(D.soft_dict(np.zeros((0, 3, 174)), np.zeros((0, 3)), [], []), code, 30, 8, 20)) == 0


@functools.lru_cache(maxsize=None)
def _oracle_records(oracle, name, seed, rf, syncmin, max_cand=D.MAX_CAND):
    iq = D.recipe_iq(name, seed)
    oc = oracle.Channel("FT4", D.FS, D.BLK, rf)
    oc.boundary(10)
    oc.push_many(iq)
    fr = oc.boundary(17)
    cands = oracle.ft4_candidates(fr["i16"], float(D.SYNC["f_lo"]), float(D.SYNC["f_hi"]), syncmin, max_cand)
    recs = oracle.ft4_sync_all(fr["i16"], cands)
    soft = D.soft_dict(*S.softbits_of_records(oracle, oracle.ft4_bigspec(fr["i16"]), recs))
    return cands, recs, soft


@pytest.mark.parametrize("seed", C.SEEDS)
def test_recipes_decode_and_reach_both_gates(oracle, seed):
    """Every transmission of every recipe yields at least one record with crc_ok in some set and exactly the 91 bits sent; at least one such
    decode needs an iteration, and one is found in set 1 after set 0 failed (the best set is not always 0); the lists' noise tails hold records
    below nsync 8 and below nqual 20, and records that pass both gates and do not decode."""
    code = C.make_code(seed)["code"]
    iters, best, sigma0 = [], [], 0
    for name, (_, _, chans) in D.RECIPES.items():
        if name in D.CARRIERS:
            continue                                                    # (no transmissions: test_carriers_frame_has_a_candidate_without_records)
        for rf, txs in chans:
            cands, recs, soft = _oracle_records(oracle, name, seed, rf, D.SYNCMIN_FT4)
            assert len(cands) < D.MAX_CAND                               # the whole list: nothing is cut at MAX_CAND
            exp = D.expected(soft, code, 30, 8, 20)
            nrec = np.bincount([r["cand"] for r in recs], minlength=len(cands))
            assert {1, 2, 3} <= set(nrec.tolist()) and len(cands) > 5   # holes in the slot array; longer than the small max_cand
            assert (soft["nsync"] < 8).any() and (soft["nqual"] < 20).any()
            assert ((soft["nsync"] >= 8) & (soft["nqual"] < 20)).any() or ((soft["nsync"] < 8) & (soft["nqual"] >= 20)).any()
            att = D.attempted(exp)
            assert (att.all(axis=1) | ~att.any(axis=1)).all() and att.any() and not att.all()
            assert (att.all(axis=1) & (D.best_set(exp) < 0)).any()
            sigma0 += int((soft["sigma"] == 0).sum())
            for audio, t0, amp, mseed in txs:
                qs = D.find_message(exp, D.message(mseed))
                assert qs, (name, rf, audio)
                b = D.best_set(exp)[qs[0]]
                best.append(int(b))
                iters.append(int(exp["set"]["iters"][qs[0], b]))
                assert abs(recs[qs[0]]["f1_hz"] - audio) <= 3.0
    assert max(iters) >= 1 and 1 in best and 0 in best, (iters, best)
    # Stated, not contrived: no record of any recipe has a set with sigma == 0 (it takes 206 equal metrics), so that gate is not exercised through
    # the chain; its comparison is the FT8 form's, which its own tests cover.
    assert sigma0 == 0


def test_carriers_frame_has_a_candidate_without_records(oracle):
    """The "carriers" recipe at HOLES_MAX_CAND: the list is cut, and its candidates have 0, 1, 2 and 3 records -- the refinement writes nrec = 0
    when all three segments stay below 1.2 -- so the slot array has a wholly empty candidate between occupied ones and the fetch's walk skips it.
    No set of these records has sigma == 0 either."""
    seed = C.SEEDS[0]
    (rf, _), = D.RECIPES["carriers"][2]
    assert len(_oracle_records(oracle, "carriers", seed, rf, D.SYNCMIN_FT4)[0]) > D.HOLES_MAX_CAND
    cands, recs, soft = _oracle_records(oracle, "carriers", seed, rf, D.SYNCMIN_FT4, D.HOLES_MAX_CAND)
    nrec = np.bincount([r["cand"] for r in recs], minlength=len(cands))
    assert len(cands) == D.HOLES_MAX_CAND and set(nrec.tolist()) == {0, 1, 2, 3} and (nrec == 0).any()
    hole = int(np.nonzero(nrec == 0)[0][0])
    assert 0 < hole < len(cands) - 1 and nrec[hole + 1:].sum() > 0     # records follow the empty candidate
    assert (soft["sigma"] != 0).all() and len(recs) == nrec.sum()


def test_quiet_threshold_empties_the_noise_channel_only(oracle):
    seed = C.SEEDS[0]
    (rf_tx, txs), (rf_noise, none) = D.RECIPES["small"][2]
    assert not none and len(_oracle_records(oracle, "small", seed, rf_noise, D.SYNCMIN_QUIET)[0]) == 0
    assert len(_oracle_records(oracle, "small", seed, rf_tx, D.SYNCMIN_QUIET)[0]) >= 1


def _header():
    src = open(os.path.join(ROOT, "include", "cwsl_gpu.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_stage_and_the_abi_version_stays():
    h = _header()
    assert re.search(r"typedef\s+struct\s*\{\s*cwslg_ft8_msg\s+set\[3\];\s*\}\s*cwslg_ft4_msg;", h)
    assert re.search(r"int\s+cwslg_enable_ft4_decode\(cwslg_ctx \*ctx, int enable, int max_iter, int min_nsync, int min_nqual\);", h)
    assert re.search(r"int\s+cwslg_fetch_ft4_decode\(cwslg_ctx \*ctx, int ch_id, cwslg_ft4_msg \*dst, int max, int \*n, uint64_t \*start_epoch\);", h)
    assert re.search(r"#define\s+CWSLG_ABI_VERSION\s+5\b", h)


def test_record_is_60_bytes_in_c_ctypes_and_numpy(tmp_path):
    from cwsl_digi_amd import api
    assert ctypes.sizeof(api.Ft4Msg) == 60 and api.FT4_MSG_DTYPE.itemsize == 60 and D.MSG4_DTYPE.itemsize == 60
    assert api.FT4_MSG_DTYPE == D.MSG4_DTYPE and api.FT4_MSG_DTYPE["set"].subdtype[0] == api.FT8_MSG_DTYPE
    src = tmp_path / "size.c"
    src.write_text('#include "cwsl_gpu.h"\n_Static_assert(sizeof(cwslg_ft4_msg) == 60, "60 bytes");\n'
                   '_Static_assert(sizeof(((cwslg_ft4_msg *)0)->set[1]) == 20, "20 bytes");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)])


def test_best_set_helper():
    from cwsl_digi_amd import api
    rec = np.zeros(4, api.FT4_MSG_DTYPE)
    rec["set"]["crc_ok"][1, 2] = 1
    rec["set"]["crc_ok"][2, 1] = rec["set"]["crc_ok"][2, 2] = 1
    rec["set"]["crc_ok"][3, 0] = 1
    assert api.ft4_best_set(rec).tolist() == [-1, 2, 1, 0] == D.best_set(rec).tolist()
    assert api.ft4_best_set(rec[2]) == 1 and api.ft4_best_set(rec[0]) == -1
    assert len(api.ft4_best_set(rec[:0])) == 0


def test_library_exports_the_symbols_and_shim_compiles():
    from cwsl_digi_amd import api
    from cwsl_digi_amd import build as B
    B.build()
    lib = ctypes.CDLL(B.LIB)
    assert hasattr(lib, "cwslg_enable_ft4_decode") and hasattr(lib, "cwslg_fetch_ft4_decode")
    assert {"cwslg_enable_ft4_decode", "cwslg_fetch_ft4_decode"} <= set(api.ABI_SYMBOLS)
    lib.cwslg_abi_version.restype = ctypes.c_int
    assert lib.cwslg_abi_version() == 5
    assert lib.cwslg_enable_ft4_decode(None, 1, 30, 8, 20) == -6 and lib.cwslg_fetch_ft4_decode(None, 0, None, 0, None, None) == -6
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", os.path.join(ROOT, "tests", "shim_ft4_decode_check.cpp")])
