"""CPU: tests/decode_reports_ref.py -- every rule of cwslg_decode_report (include/cwsl_gpu.h, "FT8 signal reports") on hand-made planes with the
answers written out -- and the re-encoder of csrc/ldpc_host.hpp (ldpc_encoder, ldpc_encode, ft8_tones_of), compiled into the stand-alone program
tests/encoder_host_check.cpp with g++ -ffp-contract=off, against tests/ldpc_cases.py and the restatement, bit for bit; once more under
-fsanitize=address,undefined."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import decode_reports_ref as RR
import ldpc_cases as LC
import report_kernel_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ZERO_WORD_TONES = np.array(list(RR.ICOS7) + [0] * 29 + list(RR.ICOS7) + [0] * 29 + list(RR.ICOS7))      # the all-zero codeword: every data tone 0


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------------------
def test_all_zero_plane():
    """xnoise 0 -> r = 0 -> -24 dB.  Tone 0 wins every tie, so the first maximum is at tone 0 everywhere: the three Costas symbols whose tone IS 0
    (the fourth of each block, 3,1,4,0,6,5,2) count for nsync, exactly as they do in cwslg_ft8_soft.nsync, and a data symbol is an error iff its
    tone is not 0."""
    pl = np.zeros((372, 32), F32)
    r = RR.report(pl, 3, 5, ZERO_WORD_TONES)
    assert (r["snr_db"], r["xsig"], r["xnoise"], r["nsync"], r["nsymerr"]) == (-24.0, 0.0, 0.0, 3, 0)
    t = ZERO_WORD_TONES.copy()
    t[[7, 8, 50]] = (1, 7, 3)
    r = RR.report(pl, 3, 5, t)
    assert (r["snr_db"], r["nsync"], r["nsymerr"]) == (-24.0, 3, 3)


def test_snr_rule():
    """r = xsig / xnoise - 1; x = r above 0.1 else 0.001; 10 log10 x - 27, not below -24: the clamp takes over below x = 10 ^ 0.3."""
    assert RR.snr_db(5.0, 0.0) == F32(-24.0) and RR.snr_db(0.0, 0.0) == F32(-24.0)          # xnoise 0 -> r = 0
    below, above = F32(1.1) - F32(2.0 ** -23), F32(1.1)                                     # r = 0.09999990 and 0.10000002 against 0.1f = 0.100000001
    assert F32(below - F32(1)) < F32(0.1) < F32(above - F32(1))
    assert RR.snr_db(below, 1.0) == F32(-24.0) and RR.snr_db(above, 1.0) == F32(-24.0)      # -57 and -37 before the clamp
    assert F32(10.0 * RR.log10_fixed(0.001) - 27.0) == F32(-57.0)
    assert RR.snr_db(2.99, 1.0) == F32(-24.0)                                               # r = 1.99: -24.0115 before the clamp
    assert RR.snr_db(3.0, 1.0) == F32(10.0 * math.log10(2.0) - 27.0) == F32(-23.9897)       # r = 2
    assert RR.snr_db(101.0, 1.0) == F32(-7.0) and RR.snr_db(1001.0, 1.0) == F32(3.0) and RR.snr_db(2002.0, 2.0) == F32(3.0)
    assert RR.snr_db(1e30, 1e-30) == F32(10.0 * RR.log10_fixed(float(np.finfo(F32).max)) - 27.0)          # an infinite ratio: the largest float's
    assert RR.snr_db(float("nan"), 1.0) == F32(-24.0) and RR.snr_db(1.0, float("nan")) == F32(-24.0)


def test_log10_fixed_is_the_oracles():
    from oracle import oracle as orc
    L = orc.lib() if hasattr(orc, "lib") else orc.L
    rng = np.random.default_rng(5)
    for x in list(10.0 ** rng.uniform(-3, 38, 400)) + [0.001, 0.1, 1.0, 2.0, float(np.finfo(F32).max)]:
        assert RR.log10_fixed(x) == L.orc_log10_fixed(x), x


def test_tie_goes_to_the_lower_tone():
    t = ZERO_WORD_TONES.copy()
    t[10], t[11] = 5, 2
    pl = np.zeros((372, 32), F32)
    i, j = 1, 0
    pl[12 + 4 * 10 - 1, i + 2 * 5] = pl[12 + 4 * 10 - 1, i + 2 * 3] = 4.0      # symbol 10: the encoded tone 5 ties with tone 3 -> the first maximum is 3
    pl[12 + 4 * 11 - 1, i + 2 * 2] = pl[12 + 4 * 11 - 1, i + 2 * 6] = 4.0      # symbol 11: the encoded tone 2 ties with tone 6 -> the first maximum is 2
    r = RR.report(pl, i, j, t)
    assert r["nsymerr"] == 1 and r["xsig"] == 8.0 and r["nsync"] == 3
    # magnitudes, not powers, are compared: two powers whose float32 roots are equal tie
    a = F32(4.0)
    b = np.nextafter(a, F32(5))
    assert a != b and np.sqrt(a, dtype=F32) == np.sqrt(b, dtype=F32)
    pl[:] = 0
    pl[12 + 4 * 10 - 1, i + 2 * 5], pl[12 + 4 * 10 - 1, i + 2 * 3] = b, a       # the encoded tone has the larger power and still loses the tie
    assert RR.report(pl, i, j, t)["nsymerr"] == 2                               # (symbol 11 now has no power at tone 2 either: first maximum 0)


def test_symbols_outside_the_plane():
    """A plane of ones: j = -62 puts symbols 0..12 before step 1, j = +62 symbols 75..78 after step 372; they contribute +0."""
    pl = np.ones((372, 32), F32)
    r = RR.report(pl, 0, -62, ZERO_WORD_TONES)
    assert (r["xsig"], r["xnoise"]) == (66.0, 66.0) and r["snr_db"] == F32(-24.0)
    r = RR.report(pl, 0, 62, ZERO_WORD_TONES)
    assert (r["xsig"], r["xnoise"]) == (75.0, 75.0)
    assert (RR.report(pl, 0, 0, ZERO_WORD_TONES)["xsig"], RR.report(pl, 0, -12, ZERO_WORD_TONES)["xsig"]) == (79.0, 78.0)


def test_tone_7_at_the_last_bin_of_the_row():
    t = ZERO_WORD_TONES.copy()
    t[20] = 7
    pl = np.zeros((372, 32), F32)
    pl[12 + 4 * 20 - 1, 31] = 9.0
    assert RR.report(pl, 17, 0, t)["xsig"] == 9.0 and RR.report(pl, 17, 0, t)["nsymerr"] == 0       # bin 17 + 14 = 31: the row's last
    assert RR.report(pl[:, :31], 17, 0, t)["xsig"] == 0.0                                            # beyond the row: +0
    big = np.zeros((372, 1936), F32)
    big[12 + 4 * 20 - 1, 1920], big[12 + 4 * 20 - 1, 1922] = 9.0, 5.0
    assert RR.report(big, 1906, 0, t)["xsig"] == 9.0                                                 # bin 1920 is the last that exists
    t[20] = 6
    t[21] = 7
    big[12 + 4 * 21 - 1, 1922] = 5.0
    assert RR.report(big, 1908, 0, t)["xsig"] == 9.0                                                 # tone 6 at bin 1920; tone 7 at 1922 is above 1920: +0


def test_sum_order():
    """Lane l adds term l + 64 to term l first; then the halves fold.  2^24 + 1 rounds back to 2^24, so the order is visible."""
    terms = np.zeros(79, F32)
    terms[0], terms[64], terms[32] = 2.0 ** 24, 1.0, 1.0
    assert RR.tree79(terms) == F32(2.0 ** 24)                                   # (2^24 + 1) + 1, each sum rounding back; 1 + 1 first would give 2^24 + 2
    terms[:] = 0
    terms[1], terms[65], terms[33], terms[0] = 1.0, 1.0, 2.0 ** 24, 0.0
    assert RR.tree79(terms) == F32(2.0 ** 24 + 2)                               # lane 1: 1 + 1 = 2 first; then 2 + 2^24 is exact
    terms[:] = 0
    terms[14], terms[78], terms[15] = 2.0 ** 24, 1.0, 1.0                       # term 78 belongs to lane 14 (2^24 + 1 rounds back), not to lane 15 (1 + 1 = 2)
    assert RR.tree79(terms) == F32(2.0 ** 24)                                   # ... and lane 15's lone 1 is lost at the last step; on lane 15: 2^24 + 2
    pl = K.plane_of_terms(0, 0, ZERO_WORD_TONES, sig=np.where(np.arange(79) == 0, 2.0 ** 24, np.where((np.arange(79) == 64) | (np.arange(79) == 32), 1, 0)).astype(F32))
    assert RR.report(pl, 0, 0, ZERO_WORD_TONES)["xsig"] == F32(2.0 ** 24)


# ---- the encoder ---------------------------------------------------------------------------------------------------------------------------------------
def _build(tmp, flags, name):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + flags + [os.path.join(ROOT, "tests", "encoder_host_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("encoder")
    return _build(tmp, [], "encoder_host_check"), _build(tmp, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "encoder_host_check_san")


def _run(exe, tmp_path, tables, words):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<I", len(tables)) + b"".join(np.asarray(t, np.uint8).tobytes() for t in tables))
        fh.write(struct.pack("<I", len(words)) + b"".join(struct.pack("<i", ti) + bytes(w) for ti, w in words))
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    tab_bytes = 8 + 2184
    assert len(raw) == len(tables) * tab_bytes + len(words) * (24 + 80)
    tabs = [(struct.unpack_from("<2i", raw, k * tab_bytes), np.frombuffer(raw, np.uint32, 546, k * tab_bytes + 8).reshape(91, 6)) for k in range(len(tables))]
    at = len(tables) * tab_bytes
    outs = [(np.frombuffer(raw, np.uint32, 6, at + k * 104), np.frombuffer(raw, np.uint8, 79, at + k * 104 + 24)) for k in range(len(words))]
    return tabs, outs


def _cw_bits(words6):
    return np.array([(int(words6[t >> 5]) >> (t & 31)) & 1 for t in range(174)], np.uint8)


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitized"])
def test_host_encoder(host_programs, tmp_path, which):
    """ldpc_host.hpp's encoder equals ldpc_cases.encode / tones_of and the restatement on seeded messages, under both codes; a table whose last 83
    columns are singular is refused by the encoder although ldpc_derive takes it; a bad table has neither."""
    rng = np.random.default_rng(77)
    tables = [LC.make_code(s)["nm"] for s in LC.SEEDS] + [K.singular_table(LC.SEEDS[0]), LC.bad_table(LC.SEEDS[0], "four_times")]
    msgs = [LC.message91(rng) for _ in range(12)] + [np.ones(91, np.uint8), np.zeros(91, np.uint8)] + [np.eye(91, dtype=np.uint8)[k] for k in (0, 63, 64, 90)]
    words = [(ti, K.word_of_bits(m)) for ti in range(4) for m in msgs]
    tabs, outs = _run(host_programs[which], tmp_path, tables, words)
    assert [t[0] for t in tabs[:3]] == [(0, 1), (0, 1), (0, 0)] and tabs[3][0][0] != 0
    assert not tabs[2][1].any() and not tabs[3][1].any()
    for ti, seed in enumerate(LC.SEEDS):
        G = RR.encoder(tables[ti])
        assert np.array_equal(tabs[ti][1], K.enc_words(G))
        assert np.array_equal(G[:, 91:], LC.make_code(seed)["P"].T)
    assert RR.encoder(tables[2]) is None
    for (ti, w), (cw, tones) in zip(words, outs):
        if ti >= 2:
            assert not cw.any() and not tones.any()
            continue
        m = RR.word_bits(np.frombuffer(w, np.uint8))
        want = LC.encode(LC.SEEDS[ti], m)
        assert np.array_equal(_cw_bits(cw), want) and np.array_equal(RR.codeword(RR.encoder(tables[ti]), np.frombuffer(w, np.uint8)), want)
        assert np.array_equal(tones, LC.tones_of(want)) and np.array_equal(RR.tones_of(want), LC.tones_of(want))


def test_tones_are_the_inverse_of_the_soft_bits_reading():
    import ft8_softbits_ref as S8
    rng = np.random.default_rng(3)
    cw = LC.encode(LC.SEEDS[0], LC.message91(rng))
    assert np.array_equal(S8.tone_bits(RR.tones_of(cw)), cw)
    assert tuple(S8.DATA_SYMBOLS) == RR.DATA and tuple(S8.COSTAS_SYMBOLS) == RR.COSTAS
