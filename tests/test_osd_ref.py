"""CPU: the numpy restatement of FT8 OSD (tests/osd_ref.py) on the test codes -- independence of the generator basis, codewords, distances by a
plain loop, the tie rule against a brute-force enumeration -- and the host header csrc/ldpc_host.hpp (generator, rank, osd_host), compiled into
the stand-alone program tests/osd_host_check.cpp with g++ -ffp-contract=off, against the restatement, bit for bit; once more under
-fsanitize=address,undefined."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def test_record_layout_and_api_surface():
    from cwsl_digi_amd import api
    for name in ("cwslg_enable_ft8_osd", "cwslg_fetch_ft8_osd", "cwslg_osd_decode"):
        assert name in api.ABI_SYMBOLS
    assert ctypes.sizeof(api.OsdMsg) == api.OSD_MSG_DTYPE.itemsize == O.OSD_DTYPE.itemsize == 24
    assert api.OSD_MSG_DTYPE == O.OSD_DTYPE
    assert [api.OSD_MSG_DTYPE.fields[n][1] for n in ("bits", "dmin", "nharderr", "nskip", "crc_ok", "how", "flip")] == [0, 12, 16, 18, 20, 21, 22]
    for name in ("enable_ft8_osd", "fetch_ft8_osd", "osd_decode"):
        assert hasattr(api.Context, name)
    assert O.NOT_ATTEMPTED.tobytes() == bytes(16) + b"\xff" * 4 + b"\x00" + b"\xff" * 3
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", os.path.join(ROOT, "tests", "shim_ft8_osd_check.cpp")])


def _mixed_basis(G, seed):
    """Another basis of the same code: the rows multiplied by a random invertible matrix over GF(2) and shuffled."""
    rng = np.random.default_rng(seed)
    while True:
        A = rng.integers(0, 2, (O.K, O.K)).astype(np.uint8)
        if O.gf2_rank(A) == O.K:
            break
    G2 = ((A.astype(int) @ G.astype(int)) % 2).astype(np.uint8)
    assert not np.array_equal(G2, G) and O.gf2_rank(G2) == O.K
    return G2


@pytest.mark.parametrize("seed", C.SEEDS)
def test_generator_spans_the_null_space(seed):
    H = C.make_code(seed)["code"].H
    G, rank = O.generator(H)
    assert rank == 83 and G.shape == (91, 174) and O.gf2_rank(G) == 91
    assert not ((H.astype(int) @ G.T.astype(int)) % 2).any()
    assert len(O.pack_generator(G)) == 2184
    # a table whose H has rank below 83: the validation takes it (every position three times), OSD cannot run on it.  Two equal rows cannot be
    # built by swapping entries without breaking the column counts, so the rank function is shown on a matrix instead
    H2 = H.copy()
    H2[1] = H2[0]
    assert O.generator(H2)[1] == 82 and O.generator(H2)[0].shape[0] == 92


@pytest.mark.parametrize("seed", C.SEEDS)
def test_result_does_not_depend_on_the_generator_basis(seed):
    """Two different bases of the same code, every set, every order: the same records; and p, nskip and the reduced basis themselves agree."""
    G = OC.generator(seed)
    G2 = _mixed_basis(G, seed)
    llr = OC.metric_sets(seed)[0]
    for order in OC.ORDERS:
        assert O.decode(G2, llr, order).tobytes() == OC.reference_records(seed, order).tobytes()
    a = np.abs(llr[OC.IDX["h2"]])
    p1, s1, g1 = O.most_reliable_basis(G, O.reliability_order(a))
    p2, s2, g2 = O.most_reliable_basis(G2, O.reliability_order(a))
    assert np.array_equal(p1, p2) and s1 == s2 and np.array_equal(g1, g2)


@pytest.mark.parametrize("seed", C.SEEDS)
def test_winners_are_codewords_with_the_stated_distance(seed):
    """H c = 0 for every winner; dmin again by a plain Python loop of numpy float32 scalars (no float64 anywhere); nharderr; the bits' packing."""
    H = C.make_code(seed)["code"].H.astype(int)
    G = OC.generator(seed).astype(int)
    llr = OC.metric_sets(seed)[0]
    for order in OC.ORDERS:
        rec = OC.reference_records(seed, order)
        for q in range(len(llr)):
            r = rec[q]
            if r["how"] == 0xff:
                assert not np.isfinite(llr[q]).all() and r.tobytes() == O.NOT_ATTEMPTED.tobytes()
                continue
            # rebuild the winner from the record's flips, independently of decode_one's candidate table
            a = np.abs(llr[q])
            hard = (llr[q] > 0).astype(np.uint8)
            p, nskip, g = O.most_reliable_basis(G, O.reliability_order(a))
            cw = (hard[p].astype(int) @ g.astype(int)) % 2
            for f in r["flip"][:r["how"]]:
                cw = cw ^ g[f]
            assert all(f == 0xff for f in r["flip"][r["how"]:]) and r["how"] <= order
            assert not ((H @ cw) % 2).any()
            assert np.array_equal(R.unpack_bits(r["bits"]), cw[:O.K]) and r["nskip"] == nskip
            d = F32(0)
            for t in range(O.N):
                if cw[t] != hard[t]:
                    d = F32(d + a[t])
            assert type(d) is F32 and d.tobytes() == r["dmin"].tobytes()
            assert r["nharderr"] == int((cw != hard).sum())
            assert r["crc_ok"] == int(R.crc14(cw[:77]) == R.crc_field(cw[:O.K]))


@pytest.mark.parametrize("seed", C.SEEDS)
def test_order_1_winner_is_minimal_under_the_tie_rule(seed):
    """Brute force at order 1: all 92 words one by one with the plain-loop distance; the winner is the minimum of (d, flips, i)."""
    G = OC.generator(seed)
    llr = OC.metric_sets(seed)[0]
    rec = OC.reference_records(seed, 1)
    for name in ("h1", "h2", "noise", "signs", "zeros", "tie"):
        q = OC.IDX[name]
        a = np.abs(llr[q])
        hard = (llr[q] > 0).astype(np.uint8)
        p, nskip, g = O.most_reliable_basis(G, O.reliability_order(a))
        c0 = ((hard[p].astype(int) @ g.astype(int)) % 2).astype(np.uint8)
        keys = []
        for k in range(92):
            cw = c0 if k == 0 else c0 ^ g[k - 1]
            d = F32(0)
            for t in np.nonzero(cw != hard)[0]:
                d = F32(d + a[t])
            keys.append((float(d), 0 if k == 0 else 1, k - 1))
        best = min(keys)
        r = rec[q]
        assert (float(r["dmin"]), int(r["how"])) == best[:2] and (r["how"] == 0 or r["flip"][0] == best[2]), (name, best, r)


# ---- csrc/ldpc_host.hpp as a stand-alone program ------------------------------------------------------------------------------------------------
def _build(tmp, flags, name):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + flags + [os.path.join(ROOT, "tests", "osd_host_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("osd")
    return _build(tmp, [], "osd_host_check"), _build(tmp, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "osd_host_check_san")


def _run(exe, tmp_path, tables, sets):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<I", len(tables)) + b"".join(np.asarray(t, np.uint8).tobytes() for t in tables))
        fh.write(struct.pack("<I", len(sets)))
        for ti, order, llr in sets:
            fh.write(struct.pack("<ii", ti, order) + np.asarray(llr, F32).tobytes())
    subprocess.check_call([exe, fin, fout])
    return open(fout, "rb").read()


def test_host_header_matches_the_restatement(host_programs, tmp_path):
    """Generator and rank of both codes and of the rejected tables; the host OSD on every set at every order under both codes."""
    tables = [C.make_code(s)["nm"] for s in C.SEEDS] + [C.bad_table(C.SEEDS[0], k) for k in C.BAD_TABLES]
    sets = [(ti, order, llr) for ti, s in enumerate(C.SEEDS) for order in OC.ORDERS for llr in OC.metric_sets(s)[0]]
    sets.append((2, 2, OC.metric_sets(C.SEEDS[0])[0][0]))                           # a rejected table: no generator, a zero record
    raws = [_run(exe, tmp_path, tables, sets) for exe in host_programs]
    assert raws[0] == raws[1]                                                       # the sanitized build ran clean and computed the same
    raw, o = raws[0], 0
    for t in tables:
        verdict, rank = struct.unpack_from("<ii", raw, o); o += 8
        blob = raw[o:o + 2184]; o += 2184
        assert verdict == R.validate(t)
        if verdict == 0:
            G, r = O.generator(R.Code(t).H)
            assert rank == r == 83 and blob == O.pack_generator(G)
        else:
            assert rank == -1 and blob == bytes(2184)
    got = np.frombuffer(raw, O.OSD_DTYPE, len(sets), o)
    assert o + 24 * len(sets) == len(raw)
    k = 0
    for s in C.SEEDS:
        for order in OC.ORDERS:
            want = OC.reference_records(s, order)
            assert got[k:k + len(want)].tobytes() == want.tobytes(), (s, order)
            k += len(want)
    assert got[k].tobytes() == bytes(24)
