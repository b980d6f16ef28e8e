"""GPU: the FT8 decode and OSD launches at many channels.  The chain tests (tests/test_gpu_ft8_decode.py, tests/test_gpu_ft8_osd.py) drive
ldpc_decode_kernel and osd_decode_kernel -- `works + blockIdx.y`, `soft[blockIdx.y]`, `msg[blockIdx.y]`, `osd[blockIdx.y]` -- with three channels;
here 37 FT8 channels (an odd count) on one 48 kHz receiver finalise in ONE boundary with soft bits, decode and OSD on, as
tests/test_gpu_softbits_scale.py::test_ft4_many_channels_one_boundary does for the soft-bit stage.  The recipe is
tests/decode_batch_cases.py's MANY_*; tests/test_decode_batch_inputs.py vets it on the CPU oracle's frames.

Standard of comparison: every decode record of the compared channels BYTE-EQUAL to ldpc_ref.hard_records on the GPU's own soft-bit records, every
OSD record BYTE-EQUAL to osd_ref.chain_records on the GPU's own soft-bit and decode records; none skipped.

Wall times: NOT YET RECORDED.  At the time of this commit the module had been collected and its inputs vetted on the CPU, but it had not run on an
MI355X; the first GPU run must record the test's wall time here (the yardstick is a few seconds; the host side -- the restatements on eight
channels' records -- takes about 2 s, measured through the CPU module).
"""
import numpy as np
import pytest

import decode_batch_cases as D
import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O

pytestmark = pytest.mark.gpu


@pytest.fixture
def xctx():
    """A fresh context in the default (exact) arithmetic mode."""
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


def _push(ctx, rx, iq):
    iq = np.ascontiguousarray(iq, dtype=np.complex64)
    for k in range(0, len(iq), 64 * D.MANY_BLK):
        ctx.push_iq(rx, iq[k:k + 64 * D.MANY_BLK])


def _same(got, want, dtype):
    assert got.dtype == want.dtype == dtype and got.shape == want.shape, (got.shape, want.shape)
    bad = [q for q in range(len(want)) if got[q].tobytes() != want[q].tobytes()]
    assert not bad, (bad[:5], [(got[q], want[q]) for q in bad[:3]])


def test_ft8_decode_and_osd_many_channels_one_boundary(xctx):
    """37 FT8 channels, max_cand 100: ldpc_decode_kernel and osd_decode_kernel run on the grid (25, 37), one launch each (sync_launches grows by
    the three launches one boundary takes with three channels).  Six probe channels (first, last, the adjacent 17 / 18, 9 and 27) carry two or
    three transmissions of real codewords at their own frequencies, start times and messages, some decoded by belief propagation, the weakened
    ones left to OSD (order 1).  On the probes and on two noise-only channels every decode and OSD record is the restatement's; each probe message
    comes out in its own channel at its own candidate from the stated stage; none of the 37 channels holds a crc_ok record, from either stage,
    with another probe's message -- a pointer table in the wrong order or with a wrong stride would put one there; the five fetches of every
    channel carry one epoch."""
    ctx = xctx
    seed, mc = D.MANY_SEED, D.MANY_SYNC["max_cand"]
    code, G = C.make_code(seed)["code"], OC.generator(seed)
    ctx.enable_sync(True, D.MANY_SYNC["syncmin"], mc, D.MANY_SYNC["f_lo"], D.MANY_SYNC["f_hi"])
    ctx.enable_ft8_softbits(True)
    ctx.set_ldpc_code(C.make_code(seed)["nm"])
    ctx.enable_ft8_decode(True, D.MANY_MAX_ITER, D.MANY_MIN_NSYNC)
    ctx.enable_ft8_osd(True, D.MANY_ORDER, D.MANY_OSD_MIN_NSYNC)
    rx = ctx.receiver_open(D.MANY_FS, D.MANY_BLK, 0)
    chans = [ctx.channel_open(rx, f, "FT8") for f in D.MANY_DIALS]
    assert len(chans) == 37
    ctx.slot_boundary("FT8", 1)
    before = ctx.stats()["sync_launches"]
    _push(ctx, rx, D.many_iq())
    ctx.slot_boundary("FT8", 16)
    ctx.synchronize()
    assert ctx.stats()["sync_launches"] - before == D.MANY_LAUNCHES       # all 37 channels in one launch of each stage
    compared = set(D.MANY_PROBES) | set(D.MANY_NOISE_ONLY)
    stages, n_msg, n_osd = set(), 0, 0
    for p, ch in enumerate(chans):
        fr = ctx.fetch_frame(ch)
        cands, t_c = ctx.fetch_candidates(ch, mc, with_epoch=True)
        llr, sigma, nsync, t_s = ctx.fetch_ft8_softbits(ch, mc, with_epoch=True)
        msg, t_m = ctx.fetch_ft8_decode(ch, mc, with_epoch=True)
        osd, t_o = ctx.fetch_ft8_osd(ch, mc, with_epoch=True)
        assert t_o == t_m == t_s == t_c == fr["t_start"] == 1, (p, t_o, t_m, t_s, t_c, fr["t_start"])
        assert len(osd) == len(msg) == len(llr) == len(cands) <= mc
        if p in compared:
            assert len(cands) > 50, (p, len(cands))
            _same(msg, R.hard_records(code, llr, D.MANY_MAX_ITER, nsync, sigma, D.MANY_MIN_NSYNC), R.MSG_DTYPE)
            _same(osd, O.chain_records(G, llr, D.MANY_ORDER, nsync, msg, D.MANY_OSD_MIN_NSYNC), O.OSD_DTYPE)
            n_msg += int((msg["iters"] >= 0).sum())
            n_osd += int((osd["how"] != 0xff).sum())
        stages |= D.assert_many_channel(p, cands, msg, osd)
        if p in D.MANY_NOISE_ONLY:
            assert not msg["crc_ok"].any() and not osd["crc_ok"].any()
    assert stages == {"bp", "osd"} and n_msg > 100 and n_osd > 100        # the comparison had attempted records of both stages to compare
