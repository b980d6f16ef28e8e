"""GPU: FT4 soft bits (cwslg_ft4_soft) through the C ABI at 48 kHz against the numpy restatement (tests/ft4_softbits_ref.py).
PARITY UNPINNED by the reference; against the restatement applied to the oracle's baseband (ft4_bigspec of the GPU's own int16 frame,
ft4_downsample at each record's f1_hz) with the GPU's own records, every record is BIT-EXACT: llr and sigma compared as uint32, nsync and
nqual as integers, every record, none skipped."""
import numpy as np
import pytest

import ft4_softbits_ref as R
from ft8_signal import ft8_iq

pytestmark = pytest.mark.gpu
FS, BLK = 48000, 1024
N4 = int(7.5 * FS) // BLK * BLK     # one FT4 slot of IQ
U32 = np.uint32


@pytest.fixture
def xctx():
    """A fresh context in the default (exact) arithmetic mode."""
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


def _iq(oracle, seed, bursts, demod_hz):
    """Weak Irwin-Hall noise plus FT4 transmissions (audio_hz, t0_s, amp, tone_seed) -> (iq, [tones])"""
    iq = oracle.synth_iq(seed, N4, FS, tones_hz=[], amp=0.0) * 0.02
    tones = []
    for audio_hz, t0, amp, ts in bursts:
        s, t = R.ft4_iq_with_tones(FS, N4, demod_hz, audio_hz, t0, amp, ts)
        iq = iq + s
        tones.append(t)
    return iq.astype(np.complex64), tones


def _run_slot(ctx, oracle, bursts, seed, demod_hz=7000, soft=True, coherent=True, max_cand=100):
    ctx.enable_sync(True, 1.5, max_cand, 200, 3000)
    ctx.enable_ft4_coherent(coherent)
    ctx.enable_ft4_softbits(soft)
    rx = ctx.receiver_open(FS, BLK, 0)
    ch = ctx.channel_open(rx, demod_hz, "FT4")
    iq, tones = _iq(oracle, seed, bursts, demod_hz)
    ctx.slot_boundary("FT4", 10); ctx.push_iq(rx, iq); ctx.slot_boundary("FT4", 17)
    return ch, tones


def _check_parity(ctx, oracle, ch, min_recs=0):
    """Frame, list, sync records and soft records of one epoch; the restatement on the oracle's baseband must equal every record, every field."""
    fr = ctx.fetch_frame(ch)
    cands, t_c = ctx.fetch_candidates(ch, with_epoch=True)
    recs = ctx.fetch_ft4_sync(ch)
    got = ctx.fetch_ft4_softbits(ch, with_epoch=True)
    assert got is not None, "no soft-bit records of the current epoch"
    llr, sigma, nsync, nqual, t_s = got
    assert t_s == t_c == fr["t_start"]
    assert recs == oracle.ft4_sync_all(fr["i16"], cands)                      # the records themselves are what they were
    cx = oracle.ft4_bigspec(fr["i16"])
    rl, rs, rn, rq = R.softbits_of_records(oracle, cx, recs)
    assert llr.shape == rl.shape == (len(recs), 3, 174) and sigma.shape == rs.shape and len(recs) >= min_recs, (llr.shape, len(recs))
    bad = np.nonzero((llr.view(U32) != rl.view(U32)).any(axis=(1, 2)) | (sigma.view(U32) != rs.view(U32)).any(axis=1) | (nsync != rn) | (nqual != rq))[0]
    assert bad.size == 0, (bad[:5], [recs[q] for q in bad[:3]])
    return dict(fr=fr, cands=cands, recs=recs, llr=llr, sigma=sigma, nsync=nsync, nqual=nqual, cx=cx)


def _best(recs, audio_hz, t0):
    near = [q for q, h in enumerate(recs) if abs(h["f1_hz"] - audio_hz) <= 2.0 and abs(h["ibest"] / 666.67 - t0) <= 0.006]
    assert near, (audio_hz, t0)
    return max(near, key=lambda q: recs[q]["sync"])


def test_three_bursts_decode_in_every_set(ctx, oracle):
    bursts = [(1000.0, 0.70, 3000.0, 51), (1900.0, 0.45, 2500.0, 52), (2600.0, 1.10, 2800.0, 53)]
    ch, tones = _run_slot(ctx, oracle, bursts, 12)
    r = _check_parity(ctx, oracle, ch, min_recs=3)
    for (audio_hz, t0, _, _), tn in zip(bursts, tones):
        q = _best(r["recs"], audio_hz, t0)
        assert r["nsync"][q] == 16 and r["nqual"][q] == 32, (audio_hz, r["nsync"][q], r["nqual"][q])
        bits = R.tone_bits(tn) == 1
        for s in range(3):
            assert np.array_equal(r["llr"][q, s] > 0, bits), (audio_hz, s, int(((r["llr"][q, s] > 0) != bits).sum()))


def test_edges_symbols_before_and_past_the_buffer(ctx, oracle):
    """One transmission that began 0.1 s before the frame (ibest < 0: leading symbols outside) and one that starts at 1.45 s
    (ibest + 3296 > 4032: trailing symbols outside): zero-filled symbols, and their set-0 metrics, come back as the restatement has them."""
    bursts = [(800.0, -0.10, 3000.0, 61), (2200.0, 1.45, 3000.0, 62)]
    ch, _ = _run_slot(ctx, oracle, bursts, 13)
    r = _check_parity(ctx, oracle, ch, min_recs=2)
    ib = np.array([h["ibest"] for h in r["recs"]])
    assert (ib < 0).any() and (ib + 3296 > 4032).any(), sorted(ib)
    # (the comparison above covers every field; here the zero-filled symbols' metrics are looked at on their own)
    for q in (int(np.argmin(ib)), int(np.argmax(ib))):
        cb = oracle.ft4_downsample(r["cx"], np.float32(r["recs"][q]["f1_hz"]))[0]
        bm = R.bitmetrics(cb.reshape(1, -1), [ib[q]])
        outside = np.array([ib[q] + 32 * k + 31 < 0 or ib[q] + 32 * k >= 4032 for k in range(103)])
        assert outside.any()
        z0 = np.repeat(outside, 2)
        assert np.array_equal(bm["bm"][0, 0][z0].view(U32), np.zeros(int(z0.sum()), U32))
        data0 = z0[R.LLR_ENTRIES]                                              # the zero metrics among the data bits: llr exactly +0
        assert np.array_equal(r["llr"][q, 0][data0].view(U32), np.zeros(int(data0.sum()), U32))
    assert (np.repeat(np.array([ib.max() + 32 * k >= 4032 for k in range(103)]), 2)[R.LLR_ENTRIES]).any()


def test_noise_only_and_cut_list(xctx, oracle):
    import cwsl_digi_amd as P
    ch, _ = _run_slot(xctx, oracle, [], 14)
    r = _check_parity(xctx, oracle, ch)                                        # n == 0 or whatever the restatement gives, no error
    assert len(r["llr"]) == len(r["recs"])
    # six bursts, max_cand = 4: the slot index 3 cand + r under a cut list
    c2 = P.Context(0)
    try:
        bursts = [(500.0 + 400.0 * j, 0.3 + 0.15 * j, 2000.0 + 300.0 * j, 70 + j) for j in range(6)]
        ch2, _ = _run_slot(c2, oracle, bursts, 15, max_cand=4)
        r2 = _check_parity(c2, oracle, ch2, min_recs=4)
        assert len(r2["cands"]) == 4 and len(oracle.ft4_candidates(r2["fr"]["i16"], 200.0, 3000.0, 1.2, 100)) > 4
        assert sorted({h["cand"] for h in r2["recs"]}) == [0, 1, 2, 3]
    finally:
        c2.close()


def test_two_ft4_channels_and_an_ft8_channel(xctx, oracle):
    from cwsl_digi_amd.api import CwslGpuError
    ctx = xctx
    fa, fb, f8 = -9000, 5000, 14000
    ba = [(900.0, 0.5, 3000.0, 81), (2100.0, 0.9, 2600.0, 82)]
    bb = [(1500.0, 0.3, 2800.0, 83)]
    iq_a, tones_a = _iq(oracle, 16, ba, fa)
    iq_b, tones_b = _iq(oracle, 17, bb, fb)
    iq = iq_a + iq_b + ft8_iq(FS, N4, f8, 1200.0, 0.4, 2500.0, np.random.default_rng(3))
    ctx.enable_sync(True, 1.5, 100, 200, 3000)
    ctx.enable_ft4_softbits(True)
    rx = ctx.receiver_open(FS, BLK, 0)
    a, b, c8 = ctx.channel_open(rx, fa, "FT4"), ctx.channel_open(rx, fb, "FT4"), ctx.channel_open(rx, f8, "FT8")
    ctx.slot_boundary("FT8", 1); ctx.slot_boundary("FT4", 10)
    ctx.push_iq(rx, iq.astype(np.complex64))
    ctx.slot_boundary("FT4", 17); ctx.slot_boundary("FT8", 16)
    ra, rb = _check_parity(ctx, oracle, a, min_recs=2), _check_parity(ctx, oracle, b, min_recs=1)
    for r, bursts, tones in ((ra, ba, tones_a), (rb, bb, tones_b)):
        for (audio_hz, t0, _, _), tn in zip(bursts, tones):
            q = _best(r["recs"], audio_hz, t0)
            assert r["nsync"][q] == 16 and np.array_equal(r["llr"][q, 0] > 0, R.tone_bits(tn) == 1)
    assert not [h for h in rb["recs"] if abs(h["f1_hz"] - 900.0) <= 2.0 and h["sync"] > 2.5]          # each channel its own records
    with pytest.raises(CwslGpuError) as e:
        ctx.fetch_ft4_softbits(c8)
    assert e.value.status == -5                                               # CWSLG_ERR_MODE


def test_life_cycle(xctx, oracle):
    from cwsl_digi_amd.api import CwslGpuError
    import cwsl_digi_amd as P
    fresh = P.Context(0)
    try:
        with pytest.raises(CwslGpuError) as e:
            fresh.enable_ft4_softbits(True)
        assert e.value.status == -6                                           # CWSLG_ERR_ARG: the sync stage is not enabled
        fresh.enable_ft4_softbits(False)                                      # switching it off is always allowed
    finally:
        fresh.close()
    ctx = xctx
    f = 7000
    slots = [_iq(oracle, 20 + k, [(700.0 + 300.0 * k, 0.4 + 0.1 * k, 3000.0, 90 + k), (2300.0 - 200.0 * k, 0.8, 2500.0, 95 + k)], f)[0] for k in range(5)]
    ctx.enable_sync(True, 1.5, 100, 200, 3000)
    rx = ctx.receiver_open(FS, BLK, 0)
    ch = ctx.channel_open(rx, f, "FT4")
    ctx.slot_boundary("FT4", 10)

    def slot(k):
        ctx.push_iq(rx, slots[k])
        ctx.slot_boundary("FT4", 17 + 7 * k)
        return 10 if k == 0 else 17 + 7 * (k - 1)                              # the start epoch of the frame just finalised

    t = slot(0)                                                               # feature never enabled
    assert ctx.fetch_ft4_softbits(ch) is None and ctx.fetch_ft4_sync(ch)
    ctx.enable_ft4_softbits(True)
    assert ctx.fetch_ft4_softbits(ch) is None                                 # enabling computes nothing by itself: from the next boundary on
    t = slot(1)                                                               # slot A
    ra = _check_parity(ctx, oracle, ch, min_recs=2)
    assert ra["fr"]["t_start"] == t and ctx.fetch_ft4_softbits(ch, with_epoch=True)[4] == t
    few = ctx.fetch_ft4_softbits(ch, max_rec=1)                               # max smaller than the count
    assert len(ra["recs"]) > 1 and few[0].shape == (1, 3, 174) and np.array_equal(few[0].view(U32), ra["llr"][:1].view(U32))
    assert np.array_equal(few[2], ra["nsync"][:1]) and np.array_equal(few[3], ra["nqual"][:1])
    ctx.enable_ft4_softbits(False)
    t = slot(2)                                                               # slot B with the feature off
    assert ctx.fetch_ft4_softbits(ch) is None                                 # not A's records under B's epoch
    assert ctx.fetch_frame(ch)["t_start"] == t and ctx.fetch_candidates(ch, with_epoch=True)[1] == t and ctx.fetch_ft4_sync(ch)
    ctx.enable_ft4_softbits(True)
    t = slot(3)
    rc = _check_parity(ctx, oracle, ch, min_recs=2)
    assert rc["fr"]["t_start"] == t and [h["f1_hz"] for h in rc["recs"]] != [h["f1_hz"] for h in ra["recs"]]
    ctx.enable_ft4_coherent(False)                                            # coherent stage off with the feature on: no records
    t = slot(4)
    assert ctx.fetch_ft4_softbits(ch) is None and ctx.fetch_candidates(ch, with_epoch=True)[1] == t


def test_no_behaviour_change_with_the_feature_on(oracle):
    import cwsl_digi_amd as P
    bursts = [(1000.0, 0.70, 3000.0, 51), (1900.0, 0.02, 2500.0, 52), (2600.0, 1.45, 2800.0, 53)]
    out = []
    for soft in (False, True):
        c = P.Context(0)
        try:
            ch, _ = _run_slot(c, oracle, bursts, 30, soft=soft)
            out.append(dict(fr=c.fetch_frame(ch)["i16"], cands=c.fetch_candidates(ch), recs=c.fetch_ft4_sync(ch),
                            cx=c.sync_debug(ch, "ft4_cx"), cd0=c.sync_debug(ch, "ft4_cd0"), soft=c.fetch_ft4_softbits(ch)))
        finally:
            c.close()
    off, on = out
    assert off["soft"] is None and on["soft"] is not None and len(on["soft"][0]) == len(on["recs"]) >= 3
    assert np.array_equal(off["fr"], on["fr"])
    bits = lambda cands: [tuple(np.float32(x).view(U32) for x in c) for c in cands]
    assert bits(off["cands"]) == bits(on["cands"]) and off["cands"]
    assert off["recs"] == on["recs"]
    assert np.array_equal(off["cx"].view(U32), on["cx"].view(U32)) and np.array_equal(off["cd0"].view(U32), on["cd0"].view(U32))
