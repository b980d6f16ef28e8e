"""CPU: FT4 soft bits -- the public declarations exist, and the numpy restatement of cwslg_ft4_soft (tests/ft4_softbits_ref.py) does what a
decoder needs: through the oracle's chain (ft4_candidates -> ft4_sync_all -> ft4_downsample at f1) a clean strong burst gives nsync = 16,
nqual = 32 and the transmitted bits in all three metric sets; the edge rules (zero fill, tail copies, all-zero input) hold exactly.
PARITY UNPINNED (no upstream source in the tree): what is checked is the stated arithmetic, not that it equals jt9's."""
import ctypes
import ctypes.util
import os
import re

import numpy as np
import pytest

import ft4_softbits_ref as R
from ft8_signal import ICOS4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U32 = np.uint32


def test_symbols_and_constants_are_declared():
    src = open(os.path.join(ROOT, "include", "cwsl_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+llr\[3\]\[174\];\s*float\s+sigma\[3\];\s*int32_t\s+nsync;\s*int32_t\s+nqual;\s*int32_t\s+pad_;\s*\}"
                     r"\s*cwslg_ft4_soft\s*;", code)
    assert re.search(r"\bint\s+cwslg_enable_ft4_softbits\s*\(\s*cwslg_ctx\s*\*\s*\w*\s*,\s*int\s+\w*\s*\)\s*;", code)
    assert re.search(r"\bint\s+cwslg_fetch_ft4_softbits\s*\(\s*cwslg_ctx\s*\*\s*\w*\s*,\s*int\s+\w*\s*,\s*cwslg_ft4_soft\s*\*\s*\w*\s*,\s*int\s+\w*\s*,"
                     r"\s*int\s*\*\s*\w*\s*,\s*uint64_t\s*\*\s*\w*\s*\)\s*;", code)
    assert "PARITY UNPINNED" in src[src.index("FT4 soft bits"):src.index("cwslg_ft4_soft;")]
    assert re.search(r"#define\s+CWSLG_ABI_VERSION\s+5\b", code)             # exports were added, nothing else changed
    from cwsl_digi_amd import api
    assert "cwslg_enable_ft4_softbits" in api.ABI_SYMBOLS and "cwslg_fetch_ft4_softbits" in api.ABI_SYMBOLS
    assert ctypes.sizeof(api.Ft4Soft) == R.RECORD_BYTES == 2112 == 4 * (3 * 174 + 3 + 3)
    assert hasattr(api.Context, "enable_ft4_softbits") and hasattr(api.Context, "fetch_ft4_softbits")
    # the four nqual patterns are the gray-decoded Costas blocks, two bits per symbol, MSB first
    inv = np.argsort(R.GRAYMAP)
    bits = np.array([[(inv[t] >> 1) & 1, inv[t] & 1] for blk in ICOS4 for t in blk]).reshape(32)
    assert np.array_equal(bits, R.QUAL_BITS)
    assert np.array_equal(R.QUAL_AT, np.concatenate([2 * 33 * b + np.arange(8) for b in range(4)]))
    assert np.array_equal(R.LLR_ENTRIES, (2 * R.DATA_SYMBOLS.reshape(-1, 1) + np.arange(2)).reshape(-1)) and len(R.LLR_ENTRIES) == 174
    # w32: (cos, +sin), cardinal points exact
    assert R.W32.dtype == np.float32 and [tuple(R.W32[p]) for p in (0, 8, 16, 24)] == [(1, 0), (0, 1), (-1, 0), (0, -1)]
    assert R.W32[1, 1] > 0 and R.W32[1, 0] == np.float32(np.cos(np.pi / 16))


def test_library_exports_the_symbols_and_shim_compiles():
    import subprocess
    from cwsl_digi_amd import build as B
    B.build()
    lib = ctypes.CDLL(B.LIB)
    assert hasattr(lib, "cwslg_enable_ft4_softbits") and hasattr(lib, "cwslg_fetch_ft4_softbits")
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", os.path.join(ROOT, "tests", "shim_ft4_softbits_check.cpp")])


def test_fmaf_is_the_single_rounding():
    """The restatement's fmaf against libm's fmaf: random operands, near-cancelling sums and ties of the double-rounding kind."""
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fmaf.restype = ctypes.c_float
    libm.fmaf.argtypes = [ctypes.c_float] * 3
    rng = np.random.default_rng(3)
    a = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 6, 4000)).astype(np.float32)
    b = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 6, 4000)).astype(np.float32)
    c = (rng.standard_normal(4000) * 10.0 ** rng.integers(-6, 6, 4000)).astype(np.float32)
    c[:1000] = -(a[:1000] * b[:1000])                       # cancellation: the result is the product's rounding error
    # double-rounding trap: a b = 1 + 2^-24 + 2^-60-ish, c tiny: float64 rounds to the float32 tie, a true fmaf does not
    a[1000:1100] = np.float32(1 + 2.0 ** -12); b[1000:1100] = np.float32(1 + 2.0 ** -12)
    c[1000:1100] = (rng.standard_normal(100) * 2.0 ** -70).astype(np.float32)
    a[1100:1200] = np.float32(0.0); c[1100:1200] = np.float32(0.0); b[1100:1150] = -b[1100:1150]
    got = R.fmaf(a, b, c)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], np.float32)
    assert np.array_equal(got.view(U32), want.view(U32))
    assert R.fmaf(np.float32(-0.0), np.float32(0.5), np.float32(0.0)).view(U32) == 0          # +0 + (-0) = +0


def test_tree_is_the_stated_order():
    rng = np.random.default_rng(0)
    b = (rng.standard_normal(206) * 1e3).astype(np.float32)
    pad = np.concatenate([b, np.zeros(50, np.float32)])
    a = [np.float32(np.float32(np.float32(pad[l] + pad[l + 64]) + pad[l + 128]) + pad[l + 192]) for l in range(64)]
    for h in (32, 16, 8, 4, 2, 1):
        for l in range(h):
            a[l] = np.float32(a[l] + a[l + h])
    assert R._tree(b.reshape(1, -1))[0].view(U32) == a[0].view(U32)


def test_one_record_spelled_out_scalar_by_scalar():
    """The vectorised restatement against loops that follow the header line by line, on a random baseband."""
    rng = np.random.default_rng(5)
    cb = (rng.standard_normal(4032) + 1j * rng.standard_normal(4032)).astype(np.complex64)
    ibest = 200
    r = R.bitmetrics(cb.reshape(1, -1), [ibest])
    f = lambda a, b, c: R.fmaf(np.float32(a), np.float32(b), np.float32(c))[()]
    g = [0, 1, 3, 2]
    cs = np.zeros((103, 4), np.complex64)
    for k in (0, 1, 2, 3, 50, 100, 101, 102):
        for q in range(4):
            zr = zi = np.float32(0)
            for t in range(32):
                c = cb[ibest + 32 * k + t]
                wx, wy = R.W32[(q * t) % 32]
                zr = f(c.real, wx, zr); zr = f(c.imag, wy, zr)
                zi = f(c.imag, wx, zi); zi = f(-c.real, wy, zi)
            assert zr.view(U32) == r["cs"][0][0, k, q].view(U32) and zi.view(U32) == r["cs"][1][0, k, q].view(U32)
            cs[k, q] = complex(zr, zi)
    mg = lambda z: np.sqrt(f(z.real, z.real, np.float32(z.imag * z.imag)))
    add = lambda x, y: np.complex64(complex(np.float32(x.real + y.real), np.float32(x.imag + y.imag)))
    # set 2, group ks = 0: metric ib pairs with index bit 7 - ib
    s2 = np.array([mg(add(add(add(cs[0, g[i >> 6]], cs[1, g[(i >> 4) & 3]]), cs[2, g[(i >> 2) & 3]]), cs[3, g[i & 3]])) for i in range(256)], np.float32)
    i = np.arange(256)
    for ib in range(8):
        on = ((i >> (7 - ib)) & 1) == 1
        assert np.float32(s2[on].max() - s2[~on].max()).view(U32) == r["bm"][0, 2, ib].view(U32)
    # set 1, pair ks = 100 -> entries 200..203; set 0 of symbol 102 -> 204, 205
    s2 = np.array([mg(add(cs[100, g[i >> 2]], cs[101, g[i & 3]])) for i in range(16)], np.float32)
    i = np.arange(16)
    for ib in range(4):
        on = ((i >> (3 - ib)) & 1) == 1
        assert np.float32(s2[on].max() - s2[~on].max()).view(U32) == r["bm"][0, 1, 200 + ib].view(U32)
    s2 = np.array([mg(cs[102, g[v]]) for v in range(4)], np.float32)
    assert np.float32(max(s2[2], s2[3]) - max(s2[0], s2[1])).view(U32) == r["bm"][0, 0, 204].view(U32)
    assert np.float32(max(s2[1], s2[3]) - max(s2[0], s2[2])).view(U32) == r["bm"][0, 0, 205].view(U32)


@pytest.fixture(scope="module")
def clean_burst(oracle):
    """One strong FT4 transmission in weak noise through the oracle's chain: frame -> candidates -> refined records -> baseband at f1."""
    frame, tones = R.ft4_frame([(1000.0, 0.7, 3000.0, 41)], 20.0, 7)
    cands = oracle.ft4_candidates(frame, 200.0, 3000.0, 1.2, 100)
    recs = oracle.ft4_sync_all(frame, cands)
    cx = oracle.ft4_bigspec(frame)
    cb = np.stack([oracle.ft4_downsample(cx, np.float32(r["f1_hz"]))[0] for r in recs])
    ib = np.array([r["ibest"] for r in recs])
    return recs, cb, ib, tones[0]


def test_clean_burst_decodes_in_all_three_sets(clean_burst):
    recs, cb, ib, tones = clean_burst
    llr, sigma, nsync, nqual = R.softbits(cb, ib)
    assert llr.shape == (len(recs), 3, 174) and llr.dtype == np.float32 and sigma.shape == (len(recs), 3)
    best = int(np.argmax([r["sync"] for r in recs]))
    assert abs(recs[best]["f1_hz"] - 1000.0) <= 2.0 and abs(recs[best]["ibest"] / 666.67 - 0.7) <= 0.006, recs[best]
    assert nsync[best] == 16 and nqual[best] == 32
    bits = R.tone_bits(tones) == 1
    for s in range(3):
        assert np.array_equal(llr[best, s] > 0, bits), (s, int(((llr[best, s] > 0) != bits).sum()))
    assert (sigma[best] > 0).all()


def test_scaling_the_baseband_scales_sigma_only(clean_burst):
    recs, cb, ib, _ = clean_burst
    a, b = R.bitmetrics(cb, ib), R.bitmetrics(cb * np.float32(2), ib)
    assert np.array_equal((a["bm"] * np.float32(2)).view(U32), b["bm"].view(U32))          # the un-normalised metrics double
    assert np.array_equal(a["nsync"], b["nsync"]) and np.array_equal(a["nqual"], b["nqual"])
    (l1, s1), (l2, s2) = R.normalise(a["bm"]), R.normalise(b["bm"])
    ulp = np.abs(l1.view(np.int32).astype(np.int64) - l2.view(np.int32).astype(np.int64))
    assert ulp.max() <= 4, int(ulp.max())
    assert np.allclose(s2, 2 * s1, rtol=1e-6)


@pytest.mark.parametrize("ibest", [-40, 4032 - 3000])
def test_symbols_outside_the_buffer_are_zero(ibest):
    rng = np.random.default_rng(9)
    cb = (rng.standard_normal(4032) + 1j * rng.standard_normal(4032)).astype(np.complex64)
    r = R.bitmetrics(cb.reshape(1, -1), [ibest])
    zr, zi = r["cs"]
    outside = np.array([ibest + 32 * k + 31 < 0 or ibest + 32 * k >= 4032 for k in range(103)])
    assert outside.any() and not outside.all()
    assert np.array_equal(zr[0, outside].view(U32), np.zeros((int(outside.sum()), 4), U32))       # exactly +0
    assert np.array_equal(zi[0, outside].view(U32), np.zeros((int(outside.sum()), 4), U32))
    assert (r["mag"][0, ~outside] > 0).all()
    bm = r["bm"][0]
    z0 = np.repeat(outside, 2)                                                 # set 0: the symbol
    z1 = np.repeat(outside[0:102:2] & outside[1:102:2], 4)                     # set 1: both symbols of the pair
    z2 = np.repeat(outside[0:100].reshape(25, 4).all(axis=1), 8)               # set 2: all four of the group
    assert np.array_equal(bm[0][z0].view(U32), np.zeros(int(z0.sum()), U32))
    assert np.array_equal(bm[1][:204][z1].view(U32), np.zeros(int(z1.sum()), U32))
    assert np.array_equal(bm[2][:200][z2].view(U32), np.zeros(int(z2.sum()), U32))
    if ibest > 0:
        assert z0.any() and z1.any() and z2.any()
    # the tails: copies of the un-normalised values
    assert np.array_equal(bm[1][204:206].view(U32), bm[0][204:206].view(U32))
    assert np.array_equal(bm[2][200:204].view(U32), bm[1][200:204].view(U32))
    assert np.array_equal(bm[2][204:206].view(U32), bm[0][204:206].view(U32))


def test_all_zero_baseband():
    llr, sigma, nsync, nqual = R.softbits(np.zeros((1, 4032), np.complex64), [300])
    assert np.array_equal(sigma.view(U32), np.zeros((1, 3), U32))
    assert np.array_equal(llr.view(U32), np.zeros((1, 3, 174), U32))            # every llr +0
    # every magnitude 0: the first maximum is tone 0, which is the Costas tone once per block; hard decisions are all 1
    assert nsync[0] == sum(row.count(0) for row in ICOS4) == 4
    assert nqual[0] == int(R.QUAL_BITS.sum()) == 16
