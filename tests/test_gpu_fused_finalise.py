"""GPU: the slot finalise fused into symbol_spectra_v2_kernel (round 6; sync_kernels.hpp, "Round 6: the slot's finalise fused ..."), on every
channel, under each of the kernel's three workgroup splits and at every edge of n_valid and of the frame's tail.

Every channel of every boundary goes through fused_finalise_check.check_slot: the int16 frame is the finalise of the GPU's own float frame bit for bit
(in exact AND in fast mode -- the arithmetic does not depend on how the float frame was made), zeros from n_valid on, and the spectra plane and the
candidate list are the restatement's on that final int16 frame.  The last two are what a window read back stale would break: both workgroups that
share samples store the same bits, so the frame in memory comes out right either way.

spectra_jper gives 62 symbol steps per workgroup at >= 512 FT8 channels per boundary, 31 at 256 .. 511, 12 below; at 512 and 600 channels (twice the
CU count) the host also picks the per-channel search kernel.  The channel counts below sit on both sides of each switch.
"""
import functools

import numpy as np
import pytest

from conftest import assert_int16_match
from ft8_signal import ft8_iq
from fused_finalise_check import FT8_COVER, SlotJobs, check_slot, spectra_jper

pytestmark = pytest.mark.gpu
FS, BLK, D = 48000, 2048, 4                      # one 48 kHz receiver block = 512 outputs; pushes are multiples of 16 samples = 4 outputs
FRAME = 240000
SYNC = dict(lo=200, hi=3000, syncmin=1.5, maxcand=200)
N_ORD = 720000 // BLK * BLK                      # an ordinary slot: 351 blocks, 718 848 samples, 179 712 outputs


def _sync_on(ctx, n_ft8):
    ctx.enable_sync(True, SYNC["syncmin"], SYNC["maxcand"], SYNC["lo"], SYNC["hi"])
    return dict(SYNC, jper=spectra_jper(n_ft8))


def _freqs(n, seed):
    return [int(f) for f in np.random.default_rng(seed).integers(-FS // 2, FS // 2 - 6500, n)]


@functools.lru_cache(maxsize=None)
def _shared_slot(oracle, seed, burst_hz):
    """One ordinary slot of IQ for a shared receiver: noise and a handful of FT8 bursts at the given dial offsets."""
    rng = np.random.default_rng(seed)
    iq = oracle.synth_iq(seed, N_ORD, FS)
    for k, f in enumerate(burst_hz):
        iq = iq + ft8_iq(FS, N_ORD, f, 500.0 + 410.0 * k + 7.0 * (seed % 13), 0.2 + 0.25 * k, 1500.0 + 300.0 * k, rng)
    return iq.astype(np.complex64)


def _push(ctx, rx, iq, oc=None):
    """The same pushes on both sides: pieces of 64 blocks, the last one as long as it is (whole blocks, then one shorter block)."""
    for k in range(0, len(iq), 64 * BLK):
        ctx.push_iq(rx, iq[k:k + 64 * BLK])
        if oc is not None:
            oc.push_stream(iq[k:k + 64 * BLK])


def _check_all(ctx, oracle, jobs, chans, sp, tag):
    for k, ch in enumerate(chans):
        jobs.submit(check_slot(ctx, oracle, ch, "FT8", sp, tag=f"{tag}/{k}"))


@pytest.mark.parametrize("n_ft8", [8, 255, 256, 300, 511, 512, 600])
def test_every_channel_under_each_split(ctx, oracle, n_ft8):
    """n_ft8 FT8 channels on one receiver, a discarded partial slot, then two emitted slots of different content (a line left over from the previous
    slot shows as wrong data, not only as zeros): every channel of both is checked in full, and only the discarded boundary ran finalize_kernel."""
    freqs = _freqs(n_ft8, 5)
    probe = tuple(freqs[k] for k in sorted({0, 1, n_ft8 // 2, n_ft8 - 1}))
    sp = _sync_on(ctx, n_ft8)
    assert sp["jper"] == (62 if n_ft8 >= 512 else 31 if n_ft8 >= 256 else 12)
    rx = ctx.receiver_open(FS, BLK, 0)
    chans = [ctx.channel_open(rx, f, "FT8") for f in freqs]
    ctx.push_iq(rx, _shared_slot(oracle, 70, probe)[:8 * BLK])
    ctx.slot_boundary("FT8", 1)                                        # partial slot: discarded
    lists = []
    with SlotJobs() as jobs:
        for s in (0, 1):
            _push(ctx, rx, _shared_slot(oracle, 71 + s, probe))
            ctx.slot_boundary("FT8", 16 + 15 * s)
            for k, ch in enumerate(chans):
                job = check_slot(ctx, oracle, ch, "FT8", sp, tag=f"{s}/channel {k}")
                g = job.fetched
                assert g["n_valid"] == N_ORD // D and g["t_start"] == 1 + 15 * s
                if freqs[k] in probe:
                    lists.append((s, k, g["cands"], g["i16"][:4000].copy()))
                jobs.submit(job)
    # the two slots differ, and the bursts were found: the checks above did not compare empty lists with empty lists
    for s, k, cands, head in lists:
        assert len(cands) >= 3, (s, k)
    a = {k: head for s, k, c, head in lists if s == 0}
    b = {k: head for s, k, c, head in lists if s == 1}
    assert all(not np.array_equal(a[k], b[k]) for k in a)
    st = ctx.stats()
    assert st["frames_emitted"] == 2 * n_ft8 and st["frames_discarded"] == n_ft8
    assert st["finalize_launches"] == 1, st["finalize_launches"]       # the discarded boundary only: both emitted slots were finalised inside the spectra kernel


# ---------------------------------------------------------------------------------------------- ragged n_valid and tails in one launch
def _ragged_lengths(jper):
    """n_valid (outputs) asked of one slot, by the path of the kernel it reaches; J = jper, seams at 480 J m.  A request is what the receiver is
    pushed; what the channel accepts is the oracle channel's fill (the last two do not fit)."""
    m = 372 // jper // 2                                               # a seam in the middle of the frame
    seam = 480 * jper * m
    return [0,                                                         # no push between two boundaries
            4, 1000,                                                   # inside the first workgroup's first windows (e0)
            100004,                                                    # = 4 mod 8: a chunk of eight straddles n_valid; off a 64-sample line
            seam - 4, seam, seam + 4,                                  # at a seam
            seam + 1440 - 4, seam + 1440 + 4,                          # inside and just past the 1440 samples two workgroups share
            179996, FT8_COVER, 180004,                                 # around `cover`, where the windows end and the tail begins
            200000,                                                    # in the tail
            239984,                                                    # the longest frame the overflow guard lets a 48 kHz channel reach (see the test)
            469 * BLK // D, 489 * BLK // D]                            # 240 128 and 250 368: to the frame's length and past it -- the guard saturates
SATURATED = 465 * BLK // D                                             # 238 080: the last whole block accepted starts at 237 568 (+ 2048 <= 239 999)


def _pushes_for(n_out, fill_limit=FRAME - 1):
    """Push lengths (samples) that bring a channel to n_out outputs.  One stream of whole blocks plus a shorter one wherever the reference's guard
    (Instance.cpp:268: fill + block > frame_len - 1 drops the block, the block counted in IQ samples) lets that through; beyond 238 080 outputs only
    ever shorter pushes are accepted: 239 984 is reached by blocks of at most fill_limit - fill samples."""
    if n_out != 239984:
        return [n_out * D] if n_out else []
    out, fill = [464 * BLK], 464 * BLK // D                            # 237 568 outputs by whole blocks
    while True:
        blk = min(BLK, (fill_limit - fill) // 16 * 16)
        if blk < 16 or fill >= n_out:
            return out
        out.append(blk); fill += blk // D


@pytest.mark.parametrize("n_ft8", [8, 300, 600])
def test_ragged_n_valid_and_tails_in_one_launch(ctx, oracle, n_ft8):
    """Private 48 kHz receivers with one FT8 channel each end their slots at different n_valid -- every edge of _ragged_lengths -- inside ONE launch,
    next to filler channels on a shared receiver that bring the boundary to n_ft8 FT8 channels (so each edge is met under each split); the next slot
    rotates the lengths, so that a channel's previous tail is longer than, shorter than and equal to the current one, and "previous tail in use,
    current slot ends before 180 000" all occur in one launch; a slot that repeats the lengths and an ordinary one follow.  After every boundary every
    channel goes through check_slot; the ragged channels also equal oracle.Channel driven with the same pushes (exact mode: the bits; fast mode: the
    +-1 LSB rule), n_valid included -- where the reference's overflow guard saturates, the oracle channel saturates with it.

    n_valid = 239 996 and 240 000 cannot be reached: the guard compares fill + block, the block counted in IQ samples, with frame_len - 1 = 239 999,
    and the shortest block is 16 samples = 4 outputs, so the last accepted block starts at fill <= 239 983, i.e. 239 980, and ends at 239 984 -- the
    longest frame there is, reached here by ever shorter pushes.  The frame's length and more are pushed all the same, as whole blocks (469 and 489 of
    them): both receivers saturate at 238 080, on both sides.  (Whole blocks, because a SHORTER block behind a dropped one is accepted by the oracle's
    push_stream, which applies the guard to every block on its own, and refused by the library, whose channel stays saturated until the boundary: the
    reference only ever has blocks of one length and does not decide between the two.)"""
    jper = spectra_jper(n_ft8)
    L = _ragged_lengths(jper)
    R = min(n_ft8, len(L))
    stride = len(L) // R                                               # 16 receivers: slot s gives receiver r the length L[r + s]; 8: L[2 r + s], four slots
    n_rot = 2 * stride
    sched = [[L[(r * stride + s) % len(L)] for r in range(R)] for s in range(n_rot)]
    sched.append(list(sched[-1]))                                      # the same lengths again: previous tail = current
    sched.append([N_ORD // D] * R)                                     # an ordinary slot
    # the schedule itself: every length occurs (twice), and every relation of previous to current end
    assert all(sum(row.count(x) for row in sched[:n_rot]) >= 2 for x in L)
    rel = set()
    for s in range(1, len(sched)):
        for r in range(R):
            prev, cur = (x if x <= 239984 else SATURATED for x in (sched[s - 1][r], sched[s][r]))
            rel.add("tail>" if prev > cur and prev > FT8_COVER and cur > FT8_COVER else "tail<" if FT8_COVER < prev < cur else
                    "tail=" if prev == cur > FT8_COVER else "tail, then short" if prev > FT8_COVER >= cur else "short")
    assert rel == {"tail>", "tail<", "tail=", "tail, then short", "short"}, rel

    sp = _sync_on(ctx, n_ft8)
    n_fill = n_ft8 - R
    fill_freqs = _freqs(n_fill, 9)
    rx_f = ctx.receiver_open(FS, BLK, 0) if n_fill else None
    fillers = [ctx.channel_open(rx_f, f, "FT8") for f in fill_freqs]
    probe = tuple(fill_freqs[:3])
    ragged = []
    for r in range(R):
        f = -20000 + 2300 * r
        rx = ctx.receiver_open(FS, BLK, 0)
        ragged.append((rx, ctx.channel_open(rx, f, "FT8"), oracle.Channel("FT8", FS, BLK, f), f))
    ctx.slot_boundary("FT8", 1)
    for rx, ch, oc, f in ragged:
        assert oc.boundary(1) is None
    reached = set()
    dropped = 0
    with SlotJobs() as jobs:
        for s, row in enumerate(sched):
            epoch = 16 + 15 * s
            if n_fill:
                _push(ctx, rx_f, _shared_slot(oracle, 200 + s, probe))
            fills = []
            for r, (rx, ch, oc, f) in enumerate(ragged):
                pushes = _pushes_for(row[r])
                n = sum(pushes)
                rng = np.random.default_rng(1000 * s + r)
                iq = oracle.synth_iq(5000 + 100 * s + r, max(n, 16), FS)
                if n > 200000:
                    iq = iq + ft8_iq(FS, len(iq), f, 700.0 + 90.0 * r, 0.3, 2000.0, rng)
                iq = iq.astype(np.complex64)
                pos = 0
                for p in pushes:
                    _push(ctx, rx, iq[pos:pos + p], oc); pos += p
                fills.append(oc.fill)
                dropped += oc.dropped
            ctx.slot_boundary("FT8", epoch)
            for r, (rx, ch, oc, f) in enumerate(ragged):
                ref = oc.boundary(epoch, want_f32=True)
                job = check_slot(ctx, oracle, ch, "FT8", sp, tag=f"{s}/receiver {r}/asked {row[r]}")
                g = job.fetched
                want_nv = row[r] if row[r] <= 239984 else SATURATED
                assert g["n_valid"] == fills[r] == want_nv, (s, r, row[r], g["n_valid"], fills[r])
                assert g["t_start"] == ref["t_start"] == epoch - 15
                if ctx.mode == "exact":
                    bad = np.nonzero(g["i16"] != ref["i16"])[0]
                    assert bad.size == 0, f"slot {s}, receiver {r}, n_valid {want_nv}: {bad.size} int16 samples differ from the oracle channel's, first at {bad[0]}"
                    assert np.float32(g["factor"]).view(np.uint32) == np.float32(ref["factor"]).view(np.uint32), (s, r, g["factor"], ref["factor"])
                else:
                    assert_int16_match(g["i16"], ref["i16"], ref["f32"] * ref["factor"])
                reached.add(want_nv)
                jobs.submit(job)
            _check_all(ctx, oracle, jobs, fillers, sp, f"{s}/filler")
    assert reached >= {x for x in L if x <= 239984} | {SATURATED}
    assert dropped > 0 and ctx.stats()["blocks_dropped"] > 0          # the guard saturated on both sides
    assert ctx.stats()["frames_emitted"] == len(sched) * n_ft8
