"""CPU: FT8 soft bits -- the public declarations exist, and the numpy restatement of cwslg_ft8_soft (tests/ft8_softbits_ref.py) decodes
synthetic frames: applied to oracle.ft8_spectra with oracle.ft8_sync's candidate list, the strongest candidate sits where the frame puts it,
all 21 Costas symbols are hard-decided right, all 174 signs are the transmitted bits, and most of the rest of the list (sidelobes, noise)
falls under ft8b's rejection rule nsync <= 6.  PARITY UNPINNED (no upstream source in the tree): what is checked is that the stated
arithmetic does what a decoder needs, not that it equals jt9's."""
import os
import re

import numpy as np
import pytest

import ft8_softbits_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared():
    src = open(os.path.join(ROOT, "include", "cwsl_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"typedef\s+struct\s*\{\s*float\s+llr\[174\];\s*float\s+sigma;\s*int32_t\s+nsync;\s*\}\s*cwslg_ft8_soft\s*;", code)
    assert re.search(r"\bint\s+cwslg_enable_ft8_softbits\s*\(\s*cwslg_ctx\s*\*\s*\w*\s*,\s*int\s+\w*\s*\)\s*;", code)
    assert re.search(r"\bint\s+cwslg_fetch_ft8_softbits\s*\(\s*cwslg_ctx\s*\*\s*\w*\s*,\s*int\s+\w*\s*,\s*cwslg_ft8_soft\s*\*\s*\w*\s*,\s*int\s+\w*\s*,"
                     r"\s*int\s*\*\s*\w*\s*,\s*uint64_t\s*\*\s*\w*\s*\)\s*;", code)
    assert "PARITY UNPINNED" in src[src.index("FT8 soft bits"):src.index("cwslg_ft8_soft;")]
    assert re.search(r"#define\s+CWSLG_ABI_VERSION\s+5\b", code)             # exports were added, nothing else changed
    import ctypes
    from cwsl_digi_amd import api
    assert "cwslg_enable_ft8_softbits" in api.ABI_SYMBOLS and "cwslg_fetch_ft8_softbits" in api.ABI_SYMBOLS
    assert ctypes.sizeof(api.Ft8Soft) == 704
    assert hasattr(api.Context, "enable_ft8_softbits") and hasattr(api.Context, "fetch_ft8_softbits")


def test_tree_is_the_stated_order():
    """The restatement's sum is the stated tree (not numpy's pairwise sum): spelled out element by element on one vector."""
    rng = np.random.default_rng(0)
    b = (rng.standard_normal(174) * 1e3).astype(np.float32)
    pad = np.concatenate([b, np.zeros(18, np.float32)])
    a = [np.float32(np.float32(pad[l] + pad[l + 64]) + pad[l + 128]) for l in range(64)]
    for h in (32, 16, 8, 4, 2, 1):
        for l in range(h):
            a[l] = np.float32(a[l] + a[l + h])
    assert R._tree(b.reshape(1, -1))[0].view(np.uint32) == a[0].view(np.uint32)


#           f0 Hz     t0 s  amp   noise seed f_hi  strongest (bin, lag)
FRAMES = [(1500.0,    0.5,  8000, 50,   1,   3000, (480, 2)),
          (1500.0,    0.5,  300,  300,  2,   3000, (480, 2)),
          (2953.125,  1.0,  8000, 50,   3,   2959, (945, 14)),
          (1000.0,    0.02, 3000, 300,  4,   3000, (320, -10))]


def _decode(oracle, f0, t0, amp, sig, seed, f_hi):
    frame, tones = R.ft8_frame(f0, t0, amp, sig, seed)
    cands = oracle.ft8_sync(frame, 200, f_hi, 1.5, 200)
    plane = oracle.ft8_spectra(frame, R.soft_pitch(f_hi))
    llr, sigma, nsync = R.softbits(plane, cands)
    return cands, tones, llr, sigma, nsync


@pytest.mark.parametrize("f0,t0,amp,sig,seed,f_hi,where", FRAMES)
def test_restatement_decodes_synthetic_frames(oracle, f0, t0, amp, sig, seed, f_hi, where):
    cands, tones, llr, sigma, nsync = _decode(oracle, f0, t0, amp, sig, seed, f_hi)
    assert len(cands) > 1 and (cands[0][0], cands[0][1]) == where, cands[:3]
    assert nsync[0] == 21
    assert np.array_equal(llr[0] > 0, R.tone_bits(tones) == 1), int(((llr[0] > 0) != (R.tone_bits(tones) == 1)).sum())
    rest = nsync[1:]
    assert 2 * int((rest <= 6).sum()) >= len(rest), (int((rest <= 6).sum()), len(rest))
    assert llr.dtype == np.float32 and sigma.dtype == np.float32 and sigma[0] > 0


def test_late_signal_bits_past_the_last_step_are_zero(oracle):
    """t0 = 2.9 s: lag >= 49, the last symbols fall past step 372 and read as 0.  Bits whose symbol lies past the last step must be exactly
    +0 -- with the search's lags (|lag| <= 62) the last DATA symbol, n = 71, ends at step 62 + 12 + 284 = 358, so that set is empty for every
    candidate a list can hold and the zero fill shows in the Costas symbols instead: here (lag 61 or 62) symbols 75..78 are past the end, their
    magnitudes are 0, and by the tie rule (first maximum) symbol 75, whose Costas tone is 0, still counts: nsync = 17 + 1."""
    frame, tones = R.ft8_frame(1500.0, 2.9, 8000, 50, 5)
    cands = oracle.ft8_sync(frame, 200, 3000, 1.5, 200)
    plane = oracle.ft8_spectra(frame, R.soft_pitch(3000))
    llr, sigma, nsync = R.softbits(plane, cands)
    assert cands[0][0] == 480 and cands[0][1] >= 49, cands[:3]
    lag = cands[0][1]
    past = R.symbols_past_end(lag)
    assert np.array_equal(llr[0][past].view(np.uint32), np.zeros(int(past.sum()), np.uint32))      # +0, bit for bit
    s8 = R.magnitudes(plane, cands[:1])[0]
    gone = (lag + 12 + 4 * np.arange(79)) > 372
    assert gone[75:].all() and not gone[:75].any(), lag
    assert np.array_equal(s8[gone].view(np.uint32), np.zeros((4, 8), np.uint32))
    assert nsync[0] == 18
    ok = ~past
    assert np.array_equal(llr[0][ok] > 0, R.tone_bits(tones)[ok] == 1)
    # a plane whose data symbols DO run past the end (a lag no search produces) gives exactly +0 there
    far = R.symbols_past_end(100)
    l2, _, _ = R.softbits(plane, [(480, 100)])
    assert far.any() and not far.all() and np.array_equal(l2[0][far].view(np.uint32), np.zeros(int(far.sum()), np.uint32))


def test_pitch_edge_tone7_at_the_old_pitch(oracle):
    """f0 = 2956.25 Hz with f_hi = 2959: bin 946, tone 7 at bin 960 = the row pitch without the feature (ib + 13 = 960); with it 992."""
    assert R.soft_pitch(2959) == 992 and (947 + 13 + 31) // 32 * 32 == 960
    # (t0 = 0.52 s rather than 0.5: at 0.5 the frame sits exactly between lags 1 and 2 and the search reports 1)
    cands, tones, llr, sigma, nsync = _decode(oracle, 2956.25, 0.52, 8000, 50, 6, 2959)
    assert (cands[0][0], cands[0][1]) == (946, 2), cands[:3]
    assert nsync[0] == 21
    assert np.array_equal(llr[0] > 0, R.tone_bits(tones) == 1)


def test_default_pitch_is_unchanged():
    assert R.soft_pitch(3000) == (960 + 13 + 31) // 32 * 32 == 992
