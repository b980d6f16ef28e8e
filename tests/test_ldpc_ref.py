"""CPU: the numpy restatement of the FT8 decode (tests/ldpc_ref.py) on the test codes (tests/ldpc_cases.py), and the host header
csrc/ldpc_host.hpp -- compiled into a stand-alone program with g++ -ffp-contract=off -- against the restatement, bit for bit."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ldpc_cases as C
import ldpc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = np.uint32
F32 = np.float32


def test_record_layout_and_api_surface():
    from cwsl_digi_amd import api
    for name in ("cwslg_set_ldpc_code", "cwslg_enable_ft8_decode", "cwslg_fetch_ft8_decode", "cwslg_ldpc_decode"):
        assert name in api.ABI_SYMBOLS
    assert ctypes.sizeof(api.Ft8Msg) == api.FT8_MSG_DTYPE.itemsize == R.MSG_DTYPE.itemsize == 20
    assert api.FT8_MSG_DTYPE == R.MSG_DTYPE
    for name in ("set_ldpc_code", "enable_ft8_decode", "fetch_ft8_decode", "ldpc_decode"):
        assert hasattr(api.Context, name)


def test_two_seeds_two_codes_of_the_stated_shape():
    a, b = (C.make_code(s) for s in C.SEEDS)
    assert not np.array_equal(a["nm"], b["nm"])
    for c in (a, b):
        nm = c["nm"]
        assert nm.shape == (83, 7) and R.validate(nm) == 0
        assert sorted((nm > 0).sum(axis=1)) == [6] * 59 + [7] * 24
        assert (np.bincount(nm[nm > 0], minlength=175)[1:] == 3).all()
        assert any(list(r[r > 0]) != sorted(r[r > 0]) for r in nm)           # entries in no particular order: the order is part of the contract
        code = c["code"]
        # per bit the three checks in ascending row order
        assert (np.diff(code.slot // 8, axis=1) > 0).all()
        for n in (0, 90, 173):
            assert [m for m in range(83) if code.H[m, n]] == list(code.slot[n] // 8)


def test_crc_is_the_stated_division():
    """The remainder of M(x) x^14 by x^14 + 0x2757, long division on integers."""
    rng = np.random.default_rng(3)
    for _ in range(20):
        b = rng.integers(0, 2, 77)
        v = int("".join(map(str, b)), 2) << (5 + 14)
        poly = 0x6757
        for sh in range(v.bit_length() - 15, -1, -1):
            if v >> (sh + 14) & 1:
                v ^= poly << sh
        assert R.crc14(b) == v
    m, bad = C.message91(rng), C.message91(rng, flip_crc=True)
    assert R.crc14(m[:77]) == R.crc_field(m) and R.crc14(bad[:77]) != R.crc_field(bad)
    assert np.array_equal(R.unpack_bits(R.pack_bits(m)), m) and R.pack_bits(m)[11] & 0x1f == 0


@pytest.mark.parametrize("seed", C.SEEDS)
def test_decodes_its_own_codewords_at_the_noise_levels(seed):
    """Ten codewords per noise level of the case list: at 0.45 and 0.62 every one decodes to the bits sent with crc_ok; at 0.8 most do, and whatever
    comes out with crc_ok is the message sent.  Clean codewords need no iteration."""
    code = C.make_code(seed)["code"]
    rng = np.random.default_rng(seed)
    msgs = [C.message91(rng) for _ in range(10)]
    cws = np.stack([C.encode(seed, m) for m in msgs])
    s = 2.0 * cws - 1.0
    clean = R.decode(code, (2.83 * s).astype(F32), 30)
    assert (clean["iters"] == 0).all() and (clean["crc_ok"] == 1).all() and (clean["nharderr"] == 0).all()
    for noise in C.NOISE_LEVELS:
        llr = (2.83 * (s + noise * rng.standard_normal(s.shape))).astype(F32)
        rec = R.decode(code, llr, 30)
        good = [q for q in range(10) if rec[q]["crc_ok"]]
        for q in good:
            assert rec[q]["nbad"] == 0 and np.array_equal(R.unpack_bits(rec[q]["bits"]), msgs[q])
            assert rec[q]["nharderr"] == int(((llr[q] > 0) != (cws[q] == 1)).sum())      # the corrected bits are the channel's errors
        assert len(good) == 10 if noise < 0.7 else len(good) >= 5, (noise, len(good))
        assert (rec["iters"] <= 30).all() and (rec["iters"][rec["nbad"] == 0] < 30).any()


@pytest.mark.parametrize("seed", C.SEEDS)
def test_random_sign_metrics_do_not_give_crc_ok(seed):
    code = C.make_code(seed)["code"]
    rng = np.random.default_rng(seed + 1)
    llr = (3.0 * (2 * rng.integers(0, 2, (40, 174)) - 1)).astype(F32)
    rec = R.decode(code, llr, 30)
    assert not rec["crc_ok"].any() and (rec["nbad"] > 0).all()
    assert (rec["iters"] >= 10).all()                                           # nothing leaves before the early stop may


def test_not_attempted_records():
    code = C.make_code(C.SEEDS[0])["code"]
    llr = C.metric_sets(C.SEEDS[0])[0][:4]
    rec = R.hard_records(code, llr, 30, nsync=[21, 6, 7, 21], sigma=[1.0, 1.0, 1.0, 0.0], min_nsync=7)
    full = C.reference_records(C.SEEDS[0], 30)
    assert rec[0] == full[0] and rec[2] == full[2]
    for q in (1, 3):
        assert rec[q]["iters"] == rec[q]["nbad"] == rec[q]["nharderr"] == -1 and rec[q]["crc_ok"] == 0 and not rec[q]["bits"].any()
        assert rec[q].tobytes() == bytes(12) + b"\xff" * 6 + bytes(2)


@pytest.mark.parametrize("kind,why", list(zip(C.BAD_TABLES, (1, 2, 2, 3, 4))))
def test_bad_tables_are_rejected(kind, why):
    for seed in C.SEEDS:
        assert R.validate(C.bad_table(seed, kind)) == why


# ---- csrc/ldpc_host.hpp as a stand-alone program ------------------------------------------------------------------------------------------------
def _tables_blob(nm):
    """LdpcTables as csrc/ldpc_host.hpp lays it out, from the restatement's derivation."""
    code = R.Code(nm)
    rowbit = np.full((128, 8), 255, np.uint8)
    rowbit[:83, :7] = np.where(code.present, code.rowbit, 255)
    epos = np.zeros((192, 4), np.uint16)
    epos[:174, :3] = code.slot
    return rowbit.tobytes() + epos.tobytes()


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ldpc") / "ldpc_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off", os.path.join(ROOT, "tests", "ldpc_host_check.cpp"), "-o", exe])
    return exe


def test_host_header_matches_the_restatement(host_program, tmp_path):
    rng = np.random.default_rng(9)
    nxt = lambda v, up: np.nextafter(F32(v), F32(np.inf if up else -np.inf), dtype=F32)
    # T: a few thousand values across the Pade range, its end at 4.97 from both sides, +-0, large values, denormals
    xs = np.concatenate([rng.uniform(-6, 6, 3000), rng.standard_normal(1000) * 0.01, [0.0, -0.0, 4.97, -4.97, 5.0, -5.0, 100.0, -1e30, np.inf, -np.inf, 1e-40, -1e-40],
                         [nxt(4.97, True), nxt(4.97, False), -nxt(4.97, True), -nxt(4.97, False)]]).astype(F32)
    # A: every breakpoint, its two neighbours, both signs; products of tanh values lie in [-1, 1]
    brk = [0.664, 0.9217, 0.9951, 0.9998, 1.0]
    ys = np.concatenate([rng.uniform(-1, 1, 3000), 1 - 10.0 ** rng.uniform(-6, -1, 1000), [0.0, -0.0], [f(b) for b in brk for f in (F32, lambda v: nxt(v, True), lambda v: nxt(v, False))]])
    ys = np.concatenate([ys, -ys]).astype(F32)
    words = rng.integers(0, 2, (300, 128)).astype(np.uint8)
    words[0] = 0
    words[1] = 1
    lohi = np.packbits(words, axis=1, bitorder="little").view("<u8")                   # bit t of the word = codeword bit t
    tables = [C.make_code(s)["nm"] for s in C.SEEDS] + [C.bad_table(s, k) for s in C.SEEDS for k in C.BAD_TABLES]
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        for arr in (xs, ys):
            fh.write(np.uint32(len(arr)).tobytes() + arr.tobytes())
        fh.write(np.uint32(len(lohi)).tobytes() + lohi.tobytes())
        fh.write(np.uint32(len(tables)).tobytes() + b"".join(np.asarray(t, np.uint8).tobytes() for t in tables))
    subprocess.check_call([host_program, fin, fout])
    raw = open(fout, "rb").read()
    o = 0
    gt = np.frombuffer(raw, F32, len(xs), o); o += 4 * len(xs)
    ga = np.frombuffer(raw, F32, len(ys), o); o += 4 * len(ys)
    gc = np.frombuffer(raw, U32, 2 * len(lohi), o).reshape(-1, 2); o += 8 * len(lohi)
    assert np.array_equal(gt.view(U32), R.T(xs).view(U32))
    assert np.array_equal(ga.view(U32), R.A(ys).view(U32))
    assert R.T(F32(-0.0)).view(U32) == 0x80000000 and R.A(F32(-0.0)).view(U32) == 0x80000000 and R.T(F32(4.97)) == 1 and R.A(F32(1.0)) == 7
    for k in range(len(lohi)):
        assert (int(gc[k, 0]), int(gc[k, 1])) == (R.crc14(words[k][:77]), R.crc_field(words[k][:91])), k
    for t in tables:
        verdict = int(np.frombuffer(raw, np.int32, 1, o)[0]); o += 4
        blob = raw[o:o + 2560]; o += 2560
        assert verdict == R.validate(t)
        assert blob == (_tables_blob(t) if verdict == 0 else bytes(2560))
    assert o == len(raw)
