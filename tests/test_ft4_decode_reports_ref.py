"""CPU: tests/ft4_decode_reports_ref.py -- every rule of the FT4 signal reports (include/cwsl_gpu.h, "FT4 signal reports") on hand-made basebands
with the answers written out -- and ft4_tones_of of csrc/ldpc_host.hpp, compiled into the stand-alone program tests/ft4_tones_host_check.cpp with
g++ -ffp-contract=off, against tests/ldpc_cases.py and the restatement, bit for bit; once more under -fsanitize=address,undefined."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import ft4_decode_cases as D
import ft4_decode_reports_ref as R4
import ft4_report_kernel_cases as K
import ft4_softbits_ref as S4
import ldpc_cases as LC
import report_kernel_cases as K8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ZERO_WORD_TONES = np.zeros(103, np.int64)
ZERO_WORD_TONES[list(R4.COSTAS)] = R4.ICOS4                             # the all-zero codeword: every data tone 0


def _amps(tones, sig=1.0, noi=0.0):
    a = np.zeros((103, 4), F32)
    a[np.arange(103), tones] = sig
    a[np.arange(103), (np.asarray(tones) + 2) & 3] = noi
    return a


# ---- the rules -----------------------------------------------------------------------------------------------------------------------------------------
def test_all_zero_baseband():
    """xnoise 0 -> r = 0 -> -21 dB.  Tone 0 wins every tie, so the first maximum is at tone 0 everywhere: the four Costas symbols whose tone IS 0
    (one per block: 0132, 1023, 2310, 3201) count for nsync, exactly as they do in cwslg_ft4_soft.nsync, and a data symbol is an error iff its
    tone is not 0."""
    cb = np.zeros(4032, np.complex64)
    r = R4.report(cb, 100, ZERO_WORD_TONES)
    assert (r["snr_db"], r["xsig"], r["xnoise"], r["nsync"], r["nsymerr"]) == (-21.0, 0.0, 0.0, 4, 0)
    assert S4.bitmetrics(cb.reshape(1, -1), [100])["nsync"][0] == 4
    t = ZERO_WORD_TONES.copy()
    t[[4, 5, 50, 98]] = (1, 3, 2, 1)
    r = R4.report(cb, 100, t)
    assert (r["snr_db"], r["nsync"], r["nsymerr"]) == (-21.0, 4, 4)
    all_ones = R4.tones(K.encoder(K.SEED), np.frombuffer(K.ALL_ONES, np.uint8))
    assert R4.report(cb, 0, all_ones)["nsymerr"] == int((all_ones[list(R4.DATA)] != 0).sum())


def test_snr_rule():
    """r = xsig / xnoise - 1; x = r above 0.1 else 0.001; 10 log10 x - 20.8, not below -21: the floor takes over below x = 10 ^ -0.02 = 0.955, so
    the 0.1 / 0.001 branch never shows."""
    assert R4.snr_db(5.0, 0.0) == F32(-21.0) and R4.snr_db(0.0, 0.0) == F32(-21.0)          # xnoise 0 -> r = 0
    below, above = F32(1.1) - F32(2.0 ** -23), F32(1.1)                                     # r = 0.09999990 and 0.10000002 against 0.1f
    assert F32(below - F32(1)) < F32(0.1) < F32(above - F32(1))
    assert R4.snr_db(below, 1.0) == F32(-21.0) and R4.snr_db(above, 1.0) == F32(-21.0)      # -50.8 and -30.8 before the floor
    assert F32(10.0 * R4.log10_fixed(0.001) - 20.8) == F32(-50.8)
    assert R4.snr_db(1.95, 1.0) == F32(-21.0)                                               # r = 0.95: -21.0228 before the floor
    assert R4.snr_db(1.96, 1.0) == F32(10.0 * R4.log10_fixed(float(F32(1.96) - F32(1))) - 20.8) and -20.99 < R4.snr_db(1.96, 1.0) < -20.97
    assert R4.snr_db(2.0, 1.0) == F32(-20.8) and R4.snr_db(101.0, 1.0) == F32(-0.8) and R4.snr_db(1001.0, 1.0) == F32(10.0 * R4.log10_fixed(1000.0) - 20.8)
    assert abs(float(R4.snr_db(1001.0, 1.0)) - 9.2) < 1e-6 and R4.snr_db(2002.0, 2.0) == R4.snr_db(1001.0, 1.0)
    assert R4.snr_db(1e30, 1e-30) == F32(10.0 * R4.log10_fixed(float(np.finfo(F32).max)) - 20.8)          # an infinite ratio: the largest float's
    assert R4.snr_db(float("nan"), 1.0) == F32(-21.0) and R4.snr_db(1.0, float("nan")) == F32(-21.0)
    assert abs(20.8 - 10.0 * math.log10(2500.0 / (12000.0 / 576.0))) < 0.01                 # the offset: reference bandwidth over a tone bin's


def test_exact_spectra_of_hand_made_basebands():
    """K.baseband_of_amps gives cs[n][q] = (amps[n][q], 0) exactly, so the rules below are tested on known powers."""
    rng = np.random.default_rng(2)
    amps = rng.integers(0, 64, (103, 4)).astype(F32) * F32(4)
    zr, zi = S4.symbol_spectra(K.baseband_of_amps(77, amps).reshape(1, -1), [77])
    assert np.array_equal(zr[0], amps) and not zi[0].any()
    r = R4.report(K.baseband_of_amps(77, _amps(ZERO_WORD_TONES, 8.0, 4.0)), 77, ZERO_WORD_TONES)
    assert (r["xsig"], r["xnoise"], r["nsync"], r["nsymerr"]) == (103 * 64.0, 103 * 16.0, 16, 0) and r["snr_db"] == R4.snr_db(4.0, 1.0)


def test_tie_goes_to_the_lower_tone():
    t = ZERO_WORD_TONES.copy()
    t[10], t[11] = 3, 1
    a = np.zeros((103, 4), F32)
    a[10, 3] = a[10, 2] = 4.0                                           # symbol 10: the encoded tone 3 ties with tone 2 -> the first maximum is 2
    a[11, 1] = a[11, 3] = 4.0                                           # symbol 11: the encoded tone 1 ties with tone 3 -> the first maximum is 1
    r = R4.report(K.baseband_of_amps(0, a), 0, t)
    assert r["nsymerr"] == 1 and r["xsig"] == 32.0 and r["nsync"] == 4 and r["xnoise"] == 16.0       # (noise: symbol 11's tone 3)
    # magnitudes, not powers, are compared: two powers whose float32 roots are equal tie
    p, q = F32(4.0), np.nextafter(F32(4.0), F32(5))
    assert p != q and np.sqrt(p, dtype=F32) == np.sqrt(q, dtype=F32)
    zr, zi = np.zeros((103, 4), F32), np.zeros((103, 4), F32)
    zr[10, 2] = 2.0                                                     # power 4
    zr[10, 3], zi[10, 3] = F32(1.2), F32(1.6)                           # the encoded tone: a slightly larger power, the same rounded root
    P = R4.powers(zr, zi)
    assert P[10, 3] > P[10, 2] and np.sqrt(P[10, 3], dtype=F32) == np.sqrt(P[10, 2], dtype=F32), P[10]
    assert R4.report_of_spectra(zr, zi, t)["nsymerr"] == 2              # it still loses the tie (symbol 11 has no power: first maximum 0, not 1)


def test_symbols_outside_the_buffer():
    """Unit amplitude at the encoded tone of every symbol (four live samples per symbol, at 0, 8, 16 and 24).  ibest = -64: symbols 0 and 1 lie
    before sample 0; ibest = 800 (ibest + 3296 > 4032): symbols 101 and 102 lie beyond sample 4031.  They read as +0: nothing for the sums, and
    a Costas symbol made of zeros still "hits" when its tone is 0 (symbols 0 and 101) and misses when it is 1 (symbols 1 and 102)."""
    amps = _amps(ZERO_WORD_TONES, 1.0)
    assert tuple(ZERO_WORD_TONES[[0, 1, 101, 102]]) == (0, 1, 0, 1)
    for ib in (-64, 800):
        r = R4.report(K.baseband_of_amps(ib, amps), ib, ZERO_WORD_TONES)
        assert (r["xsig"], r["xnoise"], r["nsync"], r["nsymerr"]) == (101.0, 0.0, 15, 0), (ib, r)
    for ib in (0, 736, 743):                                            # 743 + 32 * 102 + 24 = 4031: the last live sample is the buffer's last
        r = R4.report(K.baseband_of_amps(ib, amps), ib, ZERO_WORD_TONES)
        assert (r["xsig"], r["xnoise"], r["nsync"], r["nsymerr"]) == (103.0, 0.0, 16, 0), (ib, r)
    r = R4.report(K.baseband_of_amps(744, amps), 744, ZERO_WORD_TONES)  # one sample further: symbol 102 (tone 1) loses its last live sample
    assert (r["xsig"], r["nsync"]) == (102.5625, 16)
    # ibest = -1 cuts ONE sample off symbol 0: tone 0 keeps three quarters of its amplitude (power 0.5625) and a quarter leaks to tone 2
    r = R4.report(K.baseband_of_amps(-1, amps), -1, ZERO_WORD_TONES)
    assert (r["xsig"], r["xnoise"], r["nsync"], r["nsymerr"]) == (102.5625, 0.0625, 16, 0)
    # a data symbol beyond the buffer whose tone is not 0 is an error
    t = ZERO_WORD_TONES.copy()
    t[5] = 2
    r = R4.report(K.baseband_of_amps(-192, _amps(t, 1.0)), -192, t)    # symbols 0..5 lost
    assert (r["xsig"], r["nsync"], r["nsymerr"]) == (97.0, 13, 1)


def test_sum_order():
    """Lane l adds term l + 64 to term l first (l < 39); then the halves fold.  2^24 + 1 rounds back to 2^24, so the order is visible."""
    terms = np.zeros(103, F32)
    terms[0], terms[64], terms[32] = 2.0 ** 24, 1.0, 1.0
    assert R4.tree103(terms) == F32(2.0 ** 24)                          # (2^24 + 1) + 1, each sum rounding back; 1 + 1 first would give 2^24 + 2
    terms[:] = 0
    terms[1], terms[65], terms[33] = 1.0, 1.0, 2.0 ** 24
    assert R4.tree103(terms) == F32(2.0 ** 24 + 2)                      # lane 1: 1 + 1 = 2 first; then 2 + 2^24 is exact
    terms[:] = 0
    terms[38], terms[102], terms[39] = 2.0 ** 24, 1.0, 1.0              # term 102 belongs to lane 38 (2^24 + 1 rounds back), not to lane 39 (1 + 1 = 2)
    assert R4.tree103(terms) == F32(2.0 ** 24)
    a = np.zeros((103, 4), F32)
    a[38, 0], a[102, ZERO_WORD_TONES[102]], a[39, 0] = 4096.0, 1.0, 1.0  # powers 2^24, 1, 1 at the encoded tones
    r = R4.report(K.baseband_of_amps(5, a), 5, ZERO_WORD_TONES)
    assert r["xsig"] == F32(2.0 ** 24) and r["xnoise"] == 0.0


# ---- the tones -----------------------------------------------------------------------------------------------------------------------------------------
def test_tones_are_the_inverse_of_the_soft_bits_reading():
    rng = np.random.default_rng(3)
    for seed in LC.SEEDS:
        G = K.encoder(seed)
        for _ in range(6):
            m = LC.message91(rng)
            w = np.frombuffer(K.word_of_bits(m), np.uint8)
            cw = R4.codeword(G, w)
            assert np.array_equal(cw, LC.encode(seed, m))
            t = R4.tones(G, w)
            assert np.array_equal(S4.tone_bits(t), cw) and np.array_equal(t, D.tones_of(cw))
            assert tuple(t[list(R4.COSTAS)]) == R4.ICOS4


def _build(tmp, flags, name):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-ffp-contract=off"] + flags + [os.path.join(ROOT, "tests", "ft4_tones_host_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def host_programs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ft4_tones")
    return _build(tmp, [], "ft4_tones_host_check"), _build(tmp, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "ft4_tones_host_check_san")


def _run(exe, tmp_path, tables, words):
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as fh:
        fh.write(struct.pack("<I", len(tables)) + b"".join(np.asarray(t, np.uint8).tobytes() for t in tables))
        fh.write(struct.pack("<I", len(words)) + b"".join(struct.pack("<i", ti) + bytes(w) for ti, w in words))
    subprocess.check_call([exe, fin, fout])
    raw = open(fout, "rb").read()
    assert len(raw) == len(tables) * 8 + len(words) * (24 + 104)
    heads = [struct.unpack_from("<2i", raw, 8 * k) for k in range(len(tables))]
    at = 8 * len(tables)
    outs = [(np.frombuffer(raw, np.uint32, 6, at + k * 128), np.frombuffer(raw, np.uint8, 104, at + k * 128 + 24)) for k in range(len(words))]
    return heads, outs


@pytest.mark.parametrize("which", [0, 1], ids=["plain", "sanitized"])
def test_host_tones(host_programs, tmp_path, which):
    """ldpc_host.hpp's ft4_tones_of behind its encoder equals the restatement and ft4_decode_cases.tones_of on seeded messages, under both codes; a
    table whose last 83 columns are singular is refused by the encoder although ldpc_derive takes it; a bad table has neither."""
    rng = np.random.default_rng(78)
    tables = [LC.make_code(s)["nm"] for s in LC.SEEDS] + [K8.singular_table(LC.SEEDS[0]), LC.bad_table(LC.SEEDS[0], "four_times")]
    msgs = [LC.message91(rng) for _ in range(12)] + [np.ones(91, np.uint8), np.zeros(91, np.uint8)] + [np.eye(91, dtype=np.uint8)[k] for k in (0, 63, 64, 90)]
    words = [(ti, K.word_of_bits(m)) for ti in range(4) for m in msgs]
    heads, outs = _run(host_programs[which], tmp_path, tables, words)
    assert heads[:3] == [(0, 1), (0, 1), (0, 0)] and heads[3][0] != 0
    for (ti, w), (cw, tones) in zip(words, outs):
        if ti >= 2:
            assert not cw.any() and not tones.any()
            continue
        want = LC.encode(LC.SEEDS[ti], R4.word_bits(np.frombuffer(w, np.uint8)))
        assert np.array_equal(np.array([(int(cw[t >> 5]) >> (t & 31)) & 1 for t in range(174)], np.uint8), want)
        assert np.array_equal(tones[:103], R4.tones_of(want)) and tones[103] == 0 and np.array_equal(tones[:103], D.tones_of(want))
