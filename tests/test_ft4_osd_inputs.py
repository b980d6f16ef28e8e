"""CPU: the inputs of tests/test_gpu_ft4_osd.py, checked before any GPU sees them -- the recipes of tests/ft4_osd_cases.py on the CPU oracle's own
records (oracle.ft4_sync_all + ft4_softbits_ref.softbits_of_records) with the restatements alone (ldpc_ref, osd_ref) -- and the FT4 OSD's
surface: header, ABI version, record size in C, ctypes and numpy, the best-word helper, exports, shim.  If a property is missing the recipes
change, not these assertions."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import ft4_decode_cases as D
import ft4_osd_cases as X
import ft4_softbits_ref as S
import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATES = (X.MIN_NSYNC, X.MIN_NQUAL)


def _records(n, crc_bp=(), crc_osd=(), dtype_msg=D.MSG4_DTYPE, dtype_osd=X.OSD4_DTYPE):
    msg, osd = np.zeros(n, dtype_msg), np.zeros(n, dtype_osd)
    for q, s in crc_bp:
        msg["set"]["crc_ok"][q, s] = 1
    for q, s in crc_osd:
        osd["set"]["crc_ok"][q, s] = 1
    return msg, osd


def test_expected_applies_the_restatement_per_set_with_the_record_gate():
    """Hand-made records: a record BP decodes in set 1 alone is not attempted in ANY set (a per-set gate would attempt sets 0 and 2); a set BP did
    not attempt is not attempted; both gates; a metric that is not finite."""
    seed = C.SEEDS[0]
    G = OC.generator(seed)
    llr = OC.metric_sets(seed)[0]
    sets = llr[[OC.IDX["h1"], OC.IDX["h2"], OC.IDX["nan"]]]
    soft = D.soft_dict(np.stack([sets] * 6), np.ones((6, 3)), [8, 8, 8, 7, 8, 16], [20, 20, 20, 20, 19, 32])
    msg = np.zeros(6, D.MSG4_DTYPE)
    msg["set"]["crc_ok"][1, 1] = 1                                      # record 1: BP decoded set 1 alone
    msg["set"]["iters"][2, 0] = -1                                      # record 2: BP did not attempt set 0
    e = X.expected(soft, msg, G, 2, *GATES)
    ref = OC.reference_records(seed, 2)
    na = O.NOT_ATTEMPTED[0]
    assert e.dtype.itemsize == 72 and e["set"].shape == (6, 3)
    assert e["set"][0, 0] == ref[OC.IDX["h1"]] and e["set"][0, 1] == ref[OC.IDX["h2"]] and e["set"][0, 2] == na     # (nan: not attempted)
    assert all(e["set"][1, s] == na for s in range(3))
    assert X.per_set_gate(soft, msg, *GATES)[1].tolist() == [True, False, True] and not X.gate(soft, msg, *GATES)[1].any()
    assert e["set"][2, 0] == na and e["set"][2, 1] == ref[OC.IDX["h2"]]
    assert all(e["set"][q, s] == na for q in (3, 4) for s in range(3))  # nsync 7 < 8; nqual 19 < 20
    assert e["set"][5, 0] == ref[OC.IDX["h1"]]
    assert X.best_word(msg, e)[0].tolist() == [0, 1, 1, -1, -1, 0] and X.best_word(msg, e)[1].tolist() == [True, False, True, False, False, True]
    assert len(X.expected(D.soft_dict(np.zeros((0, 3, 174)), np.zeros((0, 3)), [], []), msg[:0], G, 2, *GATES)) == 0


@functools.lru_cache(maxsize=None)
def _oracle_records(oracle, name, seed, rf, syncmin, max_cand=X.MAX_CAND):
    iq = X.recipe_iq(name, seed)
    oc = oracle.Channel("FT4", X.FS, X.BLK, rf)
    oc.boundary(10)
    oc.push_many(iq)
    fr = oc.boundary(17)
    cands = oracle.ft4_candidates(fr["i16"], float(X.SYNC["f_lo"]), float(X.SYNC["f_hi"]), syncmin, max_cand)
    recs = oracle.ft4_sync_all(fr["i16"], cands)
    soft = D.soft_dict(*S.softbits_of_records(oracle, oracle.ft4_bigspec(fr["i16"]), recs))
    return cands, recs, soft


@functools.lru_cache(maxsize=None)
def _chain(oracle, name, seed, rf=X.RF_TX, syncmin=X.SYNCMIN_FT4, max_cand=X.MAX_CAND):
    cands, recs, soft = _oracle_records(oracle, name, seed, rf, syncmin, max_cand)
    msg = D.expected(soft, C.make_code(seed)["code"], X.MAX_ITER, *GATES)
    osd = X.expected(soft, msg, X.generator(seed), X.ORDER, *GATES)
    return cands, recs, soft, msg, osd


@pytest.mark.parametrize("seed", C.SEEDS)
def test_recipes_have_every_kind_of_record(oracle, seed):
    """Per test code, at max_iter 30, gates 8 / 20, order 2: (a) a transmission whose strongest record BP leaves without crc_ok in all three
    sets and OSD returns with exactly the 91 bits sent, with how 1 in one recipe and how 2 in another; (b) a transmission BP decodes, whose
    record OSD does not attempt; (c) a record with BP crc_ok in some but not all sets, where the record gate and a per-set gate differ;
    (d) noise-tail records below each gate, and attempted records neither stage decodes.  No false accept by OSD in any of these frames."""
    hows, partial = set(), 0
    for name in X.RECIPES:
        cands, recs, soft, msg, osd = _chain(oracle, name, seed)
        assert len(cands) < X.MAX_CAND
        bp_ok, osd_ok, att = msg["set"]["crc_ok"] != 0, osd["set"]["crc_ok"] != 0, X.attempted(osd)
        sent = {m: D.message(m) for _, _, _, m in X.transmissions(name, seed)}
        for mseed in X.RECOVERED[name][seed]:                           # (a)
            hits = X.find_word(msg, osd, sent[mseed])
            assert hits and hits[0][1], (name, mseed)
            q = hits[0][0]
            audio = [a for a, _, _, m in X.transmissions(name, seed) if m == mseed][0]
            assert abs(recs[q]["f1_hz"] - audio) <= 3.0
            assert (msg["set"]["iters"][q] >= 1).all() and not bp_ok[q].any() and att[q].all()
            # ... and BP has the word from no other record of that transmission either, the strongest included
            near = [k for k in range(len(recs)) if abs(recs[k]["f1_hz"] - audio) <= 3.0]
            assert q in near and not bp_ok[near].any()
            s = int(X.best_word(msg, osd)[0][q])
            assert osd["set"]["how"][q, s] == X.HOW[name][seed] and osd["set"]["nharderr"][q, s] > 0
            hows.add(int(osd["set"]["how"][q, s]))
        for mseed in X.BP[name][seed]:                                  # (b)
            hits = X.find_word(msg, osd, sent[mseed])
            assert hits and not hits[0][1], (name, mseed)
            assert not att[hits[0][0]].any() and all(osd["set"][hits[0][0], s] == O.NOT_ATTEMPTED[0] for s in range(3))
        some = bp_ok.any(axis=1) & ~bp_ok.all(axis=1)                   # (c)
        if X.PARTIAL.get(name, {}).get(seed):
            assert some.any(), name
            q = int(np.nonzero(some)[0][0])
            assert X.per_set_gate(soft, msg, *GATES)[q].any() and not X.gate(soft, msg, *GATES)[q].any() and not att[q].any()
        partial += int(some.sum())
        assert (soft["nsync"] < 8).any() and (soft["nqual"] < 20).any()  # (d)
        low = (soft["nsync"] < 8) | (soft["nqual"] < 20)
        assert not att[low].any() and (att.all(axis=1) | ~att.any(axis=1)).all()
        assert (att.all(axis=1) & ~osd_ok.any(axis=1)).any()            # attempted, and neither stage has a word
        assert (soft["sigma"] != 0).all() and np.isfinite(soft["llr"]).all()
        # every word either stage accepts is one that was sent
        for q in range(len(msg)):
            b, _ = X.word_bits(msg, osd, q)
            assert b is None or any(np.array_equal(b, m) for m in sent.values()), (name, q)
    assert hows == {1, 2} and partial >= 1


def test_lower_orders_find_less(oracle):
    """Order 0 and 1 on the main frame: the records differ from order 2's where the word needs more flips than the order allows."""
    seed = C.SEEDS[0]
    cands, recs, soft, msg, osd2 = _chain(oracle, "main", seed)
    G = X.generator(seed)
    osd0, osd1 = (X.expected(soft, msg, G, k, *GATES) for k in (0, 1))
    assert (X.attempted(osd0) == X.attempted(osd2)).all() and (osd0["set"]["how"][X.attempted(osd0)] == 0).all()
    assert osd1["set"]["how"][X.attempted(osd1)].max() == 1 and osd2["set"]["how"][X.attempted(osd2)].max() == 2
    assert osd0.tobytes() != osd1.tobytes() != osd2.tobytes()
    sent = D.message(X.RECOVERED["main"][seed][0])
    assert X.HOW["main"][seed] == 2 and X.find_word(msg, osd2, sent) and not X.find_word(msg, osd1, sent)


def test_carriers_frame_has_a_candidate_without_records(oracle):
    """(e) ft4_decode_cases' "carriers" frame at HOLES_MAX_CAND: a candidate with 0 records between occupied ones; at gates (0, 0) its records
    are attempted by OSD (nothing decodes by BP: no codeword is in the frame)."""
    seed = C.SEEDS[0]
    (rf, _), = D.RECIPES["carriers"][2]
    cands, recs, soft = _oracle_records(oracle, "carriers", seed, rf, X.SYNCMIN_FT4, X.HOLES_MAX_CAND)
    nrec = np.bincount([r["cand"] for r in recs], minlength=len(cands))
    assert len(cands) == X.HOLES_MAX_CAND and set(nrec.tolist()) == {0, 1, 2, 3}
    hole = int(np.nonzero(nrec == 0)[0][0])
    assert 0 < hole < len(cands) - 1 and nrec[hole + 1:].sum() > 0
    msg = D.expected(soft, C.make_code(seed)["code"], X.MAX_ITER, 0, 0)
    assert (msg["set"]["iters"] >= 0).all() and not msg["set"]["crc_ok"].any()
    assert X.gate(soft, msg, 0, 0).all()


def test_quiet_threshold_empties_the_noise_channel_only(oracle):
    """The channel without candidates: ft4_decode_cases' "small" frame (the full amplitudes) at SYNCMIN_QUIET."""
    seed = C.SEEDS[0]
    assert len(_oracle_records(oracle, "small", seed, X.RF_NOISE, X.SYNCMIN_QUIET)[0]) == 0
    assert len(_oracle_records(oracle, "small", seed, X.RF_TX, X.SYNCMIN_QUIET)[0]) >= 1


def test_rank_deficient_table_is_accepted_and_has_rank_82():
    nm = X.rank_deficient_table()
    assert R.validate(nm) == 0
    G, rank = O.generator(R.Code(nm).H)
    assert rank == 82 and G.shape[0] == 92


def _header():
    src = open(os.path.join(ROOT, "include", "cwsl_gpu.h")).read()
    return src, re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_stage_and_the_abi_version_stays():
    full, h = _header()
    assert re.search(r"typedef\s+struct\s*\{\s*cwslg_osd_msg\s+set\[3\];\s*\}\s*cwslg_ft4_osd;", h)
    assert re.search(r"int\s+cwslg_enable_ft4_osd\(cwslg_ctx \*ctx, int enable, int order, int min_nsync, int min_nqual\);", h)
    assert re.search(r"int\s+cwslg_fetch_ft4_osd\(cwslg_ctx \*ctx, int ch_id, cwslg_ft4_osd \*dst, int max, int \*n, uint64_t \*start_epoch\);", h)
    assert re.search(r"#define\s+CWSLG_ABI_VERSION\s+5\b", h)
    assert "has no OSD stage yet" not in full and re.search(r"NO\s+\*?\s*set of that record has BP crc_ok", full)
    assert "cwslg_ft4_osd" not in re.search(r"int\s+cwslg_fetch_slot\([^;]*;", h).group(0)


def test_record_is_72_bytes_in_c_ctypes_and_numpy(tmp_path):
    from cwsl_digi_amd import api
    assert ctypes.sizeof(api.Ft4Osd) == 72 and api.FT4_OSD_DTYPE.itemsize == 72 and X.OSD4_DTYPE.itemsize == 72
    assert api.FT4_OSD_DTYPE == X.OSD4_DTYPE and api.FT4_OSD_DTYPE["set"].subdtype[0] == api.OSD_MSG_DTYPE
    src = tmp_path / "size.c"
    src.write_text('#include "cwsl_gpu.h"\n_Static_assert(sizeof(cwslg_ft4_osd) == 72, "72 bytes");\n'
                   '_Static_assert(sizeof(((cwslg_ft4_osd *)0)->set[1]) == 24, "24 bytes");\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c11", "-fsyntax-only", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src)])


def test_best_word_helper():
    from cwsl_digi_amd import api
    # record 0: nothing; 1: BP set 2; 2: BP sets 1 and 2 and OSD set 0 (BP wins); 3: OSD set 1 alone; 4: OSD sets 0 and 2; 5: BP set 0 and OSD set 0
    msg, osd = _records(6, crc_bp=[(1, 2), (2, 1), (2, 2), (5, 0)], crc_osd=[(2, 0), (3, 1), (4, 0), (4, 2), (5, 0)],
                        dtype_msg=api.FT4_MSG_DTYPE, dtype_osd=api.FT4_OSD_DTYPE)
    s, by = api.ft4_best_word(msg, osd)
    assert s.tolist() == [-1, 2, 1, 1, 0, 0] and by.tolist() == [False, False, False, True, True, False]
    xs, xby = X.best_word(msg, osd)
    assert xs.tolist() == s.tolist() and xby.tolist() == by.tolist()
    assert api.ft4_best_word(msg[3], osd[3]) == (1, True) and api.ft4_best_word(msg[0], osd[0]) == (-1, False)
    assert api.ft4_best_word(msg[2], osd[2]) == (1, False)
    s0, by0 = api.ft4_best_word(msg[:0], osd[:0])
    assert len(s0) == 0 and len(by0) == 0
    assert api.ft4_best_set(msg).tolist() == [-1, 2, 1, -1, -1, 0]     # unchanged: BP alone


def test_library_exports_the_symbols_and_shim_compiles():
    from cwsl_digi_amd import api
    from cwsl_digi_amd import build as B
    B.build()
    lib = ctypes.CDLL(B.LIB)
    assert hasattr(lib, "cwslg_enable_ft4_osd") and hasattr(lib, "cwslg_fetch_ft4_osd")
    assert {"cwslg_enable_ft4_osd", "cwslg_fetch_ft4_osd"} <= set(api.ABI_SYMBOLS)
    lib.cwslg_abi_version.restype = ctypes.c_int
    assert lib.cwslg_abi_version() == 5
    assert lib.cwslg_enable_ft4_osd(None, 1, 2, 8, 20) == -6 and lib.cwslg_fetch_ft4_osd(None, 0, None, 0, None, None) == -6
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", os.path.join(ROOT, "tests", "shim_ft4_osd_check.cpp")])
