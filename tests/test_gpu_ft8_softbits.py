"""GPU: FT8 soft bits (cwslg_ft8_soft) through the C ABI at 48 kHz against the numpy restatement (tests/ft8_softbits_ref.py).
PARITY UNPINNED by the reference; against the restatement applied to oracle.ft8_spectra of the GPU's own int16 frame, with the GPU's own
(bin, lag) list, every record is BIT-EXACT: llr and sigma compared as uint32, nsync as integers, every candidate, none skipped."""
import numpy as np
import pytest

import ft8_softbits_ref as R
from ft8_signal import ft4_iq, ft8_iq

pytestmark = pytest.mark.gpu
FS, BLK = 48000, 2048
N8 = 720000 // BLK * BLK            # one FT8 slot of IQ
N4 = 360000 // BLK * BLK            # one FT4 slot
U32 = np.uint32


@pytest.fixture
def xctx():
    """A fresh context in the default (exact) arithmetic mode."""
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


def _push(ctx, rx, iq):
    iq = np.ascontiguousarray(iq, dtype=np.complex64)
    for k in range(0, len(iq), 64 * BLK):
        ctx.push_iq(rx, iq[k:k + 64 * BLK])


def _noise_iq(oracle, seed, n):
    return oracle.synth_iq(seed, n, FS)


def _signals(oracle, seed, freqs, per_channel=3, n=N8):
    """Irwin-Hall noise plus `per_channel` FT8 transmissions in each channel's passband."""
    rng = np.random.default_rng(seed)
    iq = _noise_iq(oracle, seed, n)
    for k, f in enumerate(freqs):
        for j in range(per_channel):
            iq = iq + ft8_iq(FS, n, f, 450.0 + 690.0 * j + 53.0 * k, 0.2 + 0.37 * j + 0.05 * k, 1500.0 + 500.0 * j, rng)
    return iq.astype(np.complex64)


def _check_parity(ctx, oracle, ch, f_hi=3000, min_cands=1, max_cand=600):
    """Frame, list and records of one epoch; the restatement on the oracle's plane of that frame must equal every record."""
    fr = ctx.fetch_frame(ch)
    cands, t_c = ctx.fetch_candidates(ch, max_cand, with_epoch=True)
    got = ctx.fetch_ft8_softbits(ch, max_cand, with_epoch=True)
    assert got is not None, "no soft-bit records of the current epoch"
    llr, sigma, nsync, t_s = got
    assert t_s == t_c == fr["t_start"]
    pitch = ctx.sync_debug(ch, "spectra").shape[1]
    assert pitch == R.soft_pitch(f_hi)
    plane = oracle.ft8_spectra(fr["i16"], pitch)
    rl, rs, rn = R.softbits(plane, cands)
    assert llr.shape == rl.shape == (len(cands), 174) and len(cands) >= min_cands, (llr.shape, len(cands))
    bad = np.nonzero((llr.view(U32) != rl.view(U32)).any(axis=1) | (sigma.view(U32) != rs.view(U32)) | (nsync != rn))[0]
    assert bad.size == 0, (bad[:5], [cands[q][:2] for q in bad[:5]])
    return cands, llr, sigma, nsync, fr, plane


@pytest.mark.parametrize("order", ["sync", "freq"])
def test_parity_both_orders_split_search_form(ctx, oracle, order):
    """Three channels (the search runs as ft8_sync2d_v3_kernel + ft8_candidates_kernel), both candidate orders, exact and fast demodulation."""
    freqs = [-15000, 2000, 11000]
    iq = _signals(oracle, 21, freqs)
    ctx.enable_sync(True, 1.5, 200, 200, 3000)
    ctx.set_candidate_order(order)
    ctx.enable_ft8_softbits(True)
    rx = ctx.receiver_open(FS, BLK, 0)
    chans = [ctx.channel_open(rx, f, "FT8") for f in freqs]
    ctx.slot_boundary("FT8", 1)
    _push(ctx, rx, iq)
    ctx.slot_boundary("FT8", 16)
    for ch in chans:
        cands, llr, sigma, nsync, fr, _ = _check_parity(ctx, oracle, ch, min_cands=3)
        ref = oracle.ft8_sync(fr["i16"], 200, 3000, 1.5, 200, order=order)
        assert [(c[0], c[1]) for c in cands] == [(c[0], c[1]) for c in ref]          # the lists themselves are what they were


def test_parity_per_channel_search_form(xctx, oracle):
    """520 channels on one receiver: at two workgroups' worth of channels per CU (512) a boundary runs ft8_sync_chan_kernel; the soft-bit launch
    follows it.  Channels spread over the batch are compared."""
    ctx = xctx
    rng = np.random.default_rng(5)
    freqs = [int(f) for f in rng.integers(-FS // 2, FS // 2 - 6500, 520)]
    probe = [0, 1, 257, 519]
    iq = _noise_iq(oracle, 77, N8)
    for k in probe:
        for j in range(3):
            iq = iq + ft8_iq(FS, N8, freqs[k], 400.0 + 700.0 * j + 13.0 * k % 97, 0.2 + 0.3 * j, 1500.0 + 400.0 * j, rng)
    ctx.enable_sync(True, 1.5, 100, 200, 3000)
    ctx.enable_ft8_softbits(True)
    rx = ctx.receiver_open(FS, BLK, 0)
    chans = [ctx.channel_open(rx, f, "FT8") for f in freqs]
    ctx.slot_boundary("FT8", 1)
    _push(ctx, rx, iq)
    ctx.slot_boundary("FT8", 16)
    for k in probe:
        _check_parity(ctx, oracle, chans[k], min_cands=3, max_cand=100)


def test_parity_list_cut_at_max_cand_5(xctx, oracle):
    ctx = xctx
    iq = _signals(oracle, 23, [4000], per_channel=4)
    ctx.enable_sync(True, 1.5, 5, 200, 3000)
    ctx.enable_ft8_softbits(True)
    rx = ctx.receiver_open(FS, BLK, 0)
    ch = ctx.channel_open(rx, 4000, "FT8")
    ctx.slot_boundary("FT8", 1)
    _push(ctx, rx, iq)
    ctx.slot_boundary("FT8", 16)
    cands, llr, sigma, nsync, fr, _ = _check_parity(ctx, oracle, ch, min_cands=5)
    assert len(cands) == 5 and len(oracle.ft8_sync(fr["i16"], 200, 3000, 1.5, 200)) > 5
    # a caller's own smaller `max` cuts the records like the list
    l2, s2, n2 = ctx.fetch_ft8_softbits(ch, 2)
    assert l2.shape == (2, 174) and np.array_equal(l2.view(U32), llr[:2].view(U32))


def _gauss_iq(seed, n, sigma):
    rng = np.random.default_rng(1000 + seed)
    return (rng.normal(0.0, sigma, n) + 1j * rng.normal(0.0, sigma, n)).astype(np.complex64)


def test_strongest_candidate_decodes_and_late_signal(xctx, oracle):
    """The first and fourth frames of tests/test_ft8_softbits_ref.py's table as IQ, and the late signal (t0 = 2.9 s), one channel each: the strongest
    candidate has nsync = 21 and 0 bit errors; the late one's symbols 75..78 lie past step 372, read as 0, and leave nsync = 18 (tie rule, see the
    CPU test).  Every record of every list is also the restatement's."""
    ctx = xctx
    cases = [(-9000, 1500.0, 0.5, 8000, 50, 1), (6000, 1000.0, 0.02, 3000, 300, 4), (15000, 1500.0, 2.9, 8000, 50, 5)]
    iq = np.zeros(N8, np.complex64)
    tones = []
    for f, f0, t0, amp, sig, seed in cases:
        s, t = R.ft8_iq_with_tones(FS, N8, f, f0, t0, amp, seed)
        iq = iq + s
        tones.append(t)
    iq = iq + _gauss_iq(0, N8, 300.0)
    ctx.enable_sync(True, 1.5, 200, 200, 3000)
    ctx.enable_ft8_softbits(True)
    rx = ctx.receiver_open(FS, BLK, 0)
    chans = [ctx.channel_open(rx, c[0], "FT8") for c in cases]
    ctx.slot_boundary("FT8", 1)
    _push(ctx, rx, iq)
    ctx.slot_boundary("FT8", 16)
    for k, ch in enumerate(chans):
        cands, llr, sigma, nsync, fr, plane = _check_parity(ctx, oracle, ch)
        want_bin = int(round(cases[k][1] / 3.125))
        assert cands[0][0] == want_bin, cands[:3]
        bits = R.tone_bits(tones[k]) == 1
        assert np.array_equal(llr[0] > 0, bits), (k, int(((llr[0] > 0) != bits).sum()))
        if k < 2:
            assert nsync[0] == 21
        else:
            lag = cands[0][1]
            assert lag >= 49
            gone = (lag + 12 + 4 * np.arange(79)) > 372
            assert gone[75:].all() and not gone[:75].any()
            assert nsync[0] == 18
            past = R.symbols_past_end(lag)
            assert np.array_equal(llr[0][past].view(U32), np.zeros(int(past.sum()), U32))


def test_pitch_edge_tone7_beyond_the_old_pitch(xctx, oracle):
    """f_hi = 2959: ib = 947, the row pitch without the feature is 960 and tone 7 of a candidate at bin 946 lies AT bin 960.  With the feature the
    pitch is 992, the spectra kernel fills every bin below it (compared with the restatement's plane) and the records are the restatement's."""
    ctx = xctx
    f = 3000
    s, tones = R.ft8_iq_with_tones(FS, N8, f, 2956.25, 0.52, 8000, 6)
    iq = s + _gauss_iq(6, N8, 50.0)
    ctx.enable_sync(True, 1.5, 200, 200, 2959)
    ctx.enable_ft8_softbits(True)
    rx = ctx.receiver_open(FS, BLK, 0)
    ch = ctx.channel_open(rx, f, "FT8")
    ctx.slot_boundary("FT8", 1)
    _push(ctx, rx, iq)
    ctx.slot_boundary("FT8", 16)
    cands, llr, sigma, nsync, fr, plane = _check_parity(ctx, oracle, ch, f_hi=2959)
    g = ctx.sync_debug(ch, "spectra")
    assert g.shape == (372, 992) and np.array_equal(g.view(U32), plane.view(U32))
    assert cands[0][0] in (946, 947), cands[:3]
    edge = [q for q, c in enumerate(cands) if c[0] in (946, 947)]
    s8 = R.magnitudes(plane, [cands[q] for q in edge])
    assert (s8[:, :, 7] > 0).any()                                   # tone 7 (bins 960 / 961) carries energy: it is read, not zero-filled
    if cands[0][0] == 946:
        assert nsync[0] == 21 and np.array_equal(llr[0] > 0, R.tone_bits(tones) == 1)


def test_silent_channel_and_ft4_channel(xctx, oracle):
    """A silent FT8 channel gives n = 0 without an error; on an FT4 channel of the same context the fetch is CWSLG_ERR_MODE and the FT4 results are
    what a context without the feature computes."""
    from cwsl_digi_amd.api import CwslGpuError
    import cwsl_digi_amd as P
    rng = np.random.default_rng(8)
    f8, f8s, f4 = 9000, -3000, -14000
    iq = _noise_iq(oracle, 31, N8)
    # (the silent channel sits on a receiver of its own that is fed zeros)
    for j in range(2):
        iq = iq + ft8_iq(FS, N8, f8, 700.0 + 800.0 * j, 0.3 + 0.4 * j, 2000.0, rng)
        iq = iq + ft4_iq(FS, N8, f4, 900.0 + 700.0 * j, 0.3 + 0.2 * j, 2500.0, rng)
    iq = iq.astype(np.complex64)

    def run(c, soft):
        c.enable_sync(True, 1.5, 200, 200, 3000)
        if soft:
            c.enable_ft8_softbits(True)
        rx, rx0 = c.receiver_open(FS, BLK, 0), c.receiver_open(FS, BLK, 0)
        a, b, s = c.channel_open(rx, f8, "FT8"), c.channel_open(rx, f4, "FT4"), c.channel_open(rx0, f8s, "FT8")
        c.slot_boundary("FT8", 1)
        c.slot_boundary("FT4", 1)
        _push(c, rx, iq[:N4])
        _push(c, rx0, np.zeros(N4, np.complex64))
        c.slot_boundary("FT4", 8)
        _push(c, rx, iq[N4:])
        _push(c, rx0, np.zeros(N8 - N4, np.complex64))
        c.slot_boundary("FT8", 16)
        return a, b, s

    ctx = xctx
    a, b, s = run(ctx, True)
    _check_parity(ctx, oracle, a, min_cands=2)
    llr, sigma, nsync = ctx.fetch_ft8_softbits(s)
    assert llr.shape == (0, 174) and len(sigma) == 0 and len(nsync) == 0 and ctx.fetch_candidates(s) == []
    with pytest.raises(CwslGpuError) as e:
        ctx.fetch_ft8_softbits(b)
    assert e.value.status == -5                                       # CWSLG_ERR_MODE
    plain = P.Context(0)
    try:
        a2, b2, s2 = run(plain, False)
        assert np.array_equal(plain.fetch_frame(b2)["i16"], ctx.fetch_frame(b)["i16"])
        c1, c2 = ctx.fetch_candidates(b), plain.fetch_candidates(b2)
        assert len(c1) >= 2 and [tuple(np.float32(x).view(U32) for x in c) for c in c1] == [tuple(np.float32(x).view(U32) for x in c) for c in c2]
        assert ctx.fetch_ft4_sync(b) == plain.fetch_ft4_sync(b2) and len(ctx.fetch_ft4_sync(b)) >= 1
        assert plain.fetch_ft8_softbits(a2) is None                   # never enabled: CWSLG_ERR_NO_FRAME
        assert ctx.fetch_candidates(a) == plain.fetch_candidates(a2)  # and the FT8 list does not depend on the feature
    finally:
        plain.close()


def test_enable_needs_the_sync_stage(xctx):
    from cwsl_digi_amd.api import CwslGpuError
    with pytest.raises(CwslGpuError) as e:
        xctx.enable_ft8_softbits(True)
    assert e.value.status == -6                                       # CWSLG_ERR_ARG
    xctx.enable_ft8_softbits(False)                                   # switching it off is always allowed


def test_epochs_and_off_means_off(xctx, oracle):
    """Five consecutive slots of one channel, f_hi = 2959 (row pitch 960 without the feature, 992 with it):
    1 sync on, soft bits never enabled: nothing to fetch; launches per boundary and row pitch noted;
    2, 3 enabled, different signals: the records fetched after slot 3 are slot 3's, under the epoch of the list and the frame;
    4 disabled: the fetch is CWSLG_ERR_NO_FRAME -- not slot 3's records under slot 4's epoch -- and launches and pitch are slot 1's;
    5 enabled again: records of slot 5."""
    ctx = xctx
    f = -5000
    rng = np.random.default_rng(12)
    slots = []
    for k in range(5):
        iq = _noise_iq(oracle, 40 + k, N8)
        for j in range(2):
            iq = iq + ft8_iq(FS, N8, f, 500.0 + 410.0 * j + 170.0 * k, 0.2 + 0.3 * j + 0.1 * k, 2000.0, rng)
        slots.append(iq.astype(np.complex64))
    ctx.enable_sync(True, 1.5, 200, 200, 2959)
    rx = ctx.receiver_open(FS, BLK, 0)
    ch = ctx.channel_open(rx, f, "FT8")
    ctx.slot_boundary("FT8", 1)

    def slot(k):
        before = ctx.stats()["sync_launches"]
        _push(ctx, rx, slots[k])
        ctx.slot_boundary("FT8", 16 + 15 * k)
        ctx.synchronize()
        return ctx.stats()["sync_launches"] - before, ctx.sync_debug(ch, "spectra").shape[1]

    off = slot(0)
    assert off == (1, 960)
    assert ctx.fetch_ft8_softbits(ch) is None
    assert [c[:2] for c in ctx.fetch_candidates(ch)] == [c[:2] for c in oracle.ft8_sync(ctx.fetch_frame(ch)["i16"], 200, 2959, 1.5, 200)]
    ctx.enable_ft8_softbits(True)
    assert slot(1) == (1, 992)
    first = _check_parity(ctx, oracle, ch, f_hi=2959, min_cands=2)
    assert slot(2) == (1, 992)
    second = _check_parity(ctx, oracle, ch, f_hi=2959, min_cands=2)
    assert second[4]["t_start"] == 16 + 15 and first[4]["t_start"] == 16
    assert [c[:2] for c in first[0]] != [c[:2] for c in second[0]]    # different signals: slot 2's records would not pass for slot 3
    ctx.enable_ft8_softbits(False)
    assert slot(3) == off
    assert ctx.fetch_ft8_softbits(ch) is None
    cands, t_c = ctx.fetch_candidates(ch, with_epoch=True)
    assert t_c == 16 + 30 and len(cands) >= 2                         # the list of slot 4 is there; the records are not
    ctx.enable_ft8_softbits(True)
    assert ctx.fetch_ft8_softbits(ch) is None                         # enabling computes nothing by itself: from the next boundary on
    assert slot(4) == (1, 992)
    last = _check_parity(ctx, oracle, ch, f_hi=2959, min_cands=2)
    assert last[4]["t_start"] == 16 + 45
