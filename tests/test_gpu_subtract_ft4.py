"""GPU: cwslg_subtract_ft4 on the chain (include/cwsl_gpu.h, "FT4 signal subtraction") -- 3 FT4 channels x 1 slot, the smallest group that has a
channel with several decodes, one with one and one with none.  Every comparison is byte for byte: `dec` against cwslg_fetch_decodes, `sub` and every
residual against tests/ft4_subtract_ref.py applied to the GPU's own float frame (cwslg_fetch_audio_f32) and `dec`.
On fresh contexts: a slot that ends early after two full ones (the n_valid masks against a stale tail), every `max` from 0 to beyond the total, and
nine channels opened after a first call (the residual block made anew).  Times on one MI355X, the restatement on the host included:
test_slot_against_the_restatement 0.14 s; the short slot 0.16, every max 0.20, the grown block 0.16 s."""
import ctypes as C

import numpy as np
import pytest

import ft4_decode_report_cases as RC4
import ft4_decode_reports_ref as R4
import ft4_subtract_ref as S
import ldpc_cases as LC
import record_race_cases as RC
import report_kernel_cases as K

pytestmark = pytest.mark.gpu
NO_FRAME, ERR_ARG = -9, -6
BIG = 1 << 16
MODE = "FT4"
SEED = RC4.SEED
# The slot is ft4_decode_report_cases' slot 0 (nine transmissions on its first dial offset, tests/test_ft4_decode_reports_inputs.py proves what it
# contains).  Dial offsets here: its first channel (several decodes); the same 2500 Hz lower, which puts the 300 Hz transmission at 2800 Hz and
# every other one above the 3000 Hz end of the search band (one decode; on the CPU chain of restatements: one, at 2800.3 Hz, dt 0.301 s); its
# second channel, which hears noise (none)
RFS = (RC4.RF[0], RC4.RF[0] - 2500, RC4.RF[1])
E0 = RC4.start_epoch(0)


def _open(ctx, seed=SEED, code=None):
    s = RC.SYNC
    ctx.enable_sync(True, s["syncmin"], 100, s["f_lo"], s["f_hi"])
    ctx.set_ft4_syncmin(RC.SYNCMIN_FT4)
    ctx.set_ldpc_code(LC.make_code(seed)["nm"] if code is None else code)
    ctx.enable_ft4_softbits(True)
    ctx.enable_ft4_decode(True, *RC.DECODE4)
    ctx.enable_ft4_osd(True, *RC.OSD4)
    rx = ctx.receiver_open(RC4.FS, RC4.BLK, 0)
    chans = [ctx.channel_open(rx, rf, MODE) for rf in RFS]
    ctx.slot_boundary(MODE, E0)
    return rx, chans


def _slot(ctx, rx, e, n_blocks=None):
    """n_blocks: a slot that ends early, after that many receiver blocks of IQ"""
    iq, step = RC4.slot_iq(0), 64 * RC4.BLK                              # (every slot carries the same IQ: the epochs differ, which is what matters here)
    if n_blocks is not None:
        iq = iq[:n_blocks * RC4.BLK]
    for k in range(0, len(iq), step):
        ctx.push_iq(rx, iq[k:k + step])
    ctx.slot_boundary(MODE, RC4.start_epoch(e + 1))


@pytest.fixture(scope="module")
def slot():
    """(ctx, rx, chans) with slot 0 decoded; the tests below only fetch, except the last one of the file, which fires the next boundary"""
    import cwsl_digi_amd as P
    c = P.Context(0)
    rx, chans = _open(c)
    _slot(c, rx, 0)
    yield c, rx, chans
    c.close()


_REF = {}


def _want(ctx, chans, dec, key):
    """the restatement on the GPU's own frames and `dec`: (sub, {ch: residual}); computed once per (frame set, max) and shared"""
    if key in _REF:
        return _REF[key]
    G = K.encoder(SEED)
    sub = np.zeros(len(dec), S.SUB_DTYPE)
    res = {}
    for ch in chans:
        audio, nv = ctx.fetch_audio_f32(ch)             # (the decoder's frame is the first 72576 samples of the device's)
        assert audio.size >= S.N and not audio[nv:].any()
        audio = audio[:S.N]
        idx = np.flatnonzero(dec["ch_id"] == ch)
        recs, res[ch], _ = S.subtract(audio, [(R4.tones(G, dec["bits"][i]), dec["freq_hz"][i], dec["dt_s"][i]) for i in idx])
        sub[idx] = recs
    _REF[key] = (sub, res)
    return _REF[key]


def _check(ctx, chans, mx, key):
    plain = ctx.fetch_decodes(MODE, 0, mx)
    got = ctx.subtract_ft4(0, mx)
    dec, sub, E, n_total, n_ch = got
    assert (E, n_total, n_ch) == plain[1:] and dec.tobytes() == plain[0].tobytes() and len(sub) == len(dec) == min(n_total, mx)
    want_sub, want_res = _want(ctx, chans, dec, key)
    bad = [p for p in range(len(dec)) if sub[p].tobytes() != want_sub[p].tobytes()]
    assert not bad, (bad[:5], sub[bad[:3]], want_sub[bad[:3]])
    for ch in chans:
        r, e = ctx.fetch_ft4_residual(ch)
        assert e == E and r.size == S.N
        diff = np.flatnonzero(r.view(np.uint32) != want_res[ch].view(np.uint32))
        assert diff.size == 0, (ch, diff.size, diff[:5])
    return got


def test_slot_against_the_restatement(slot):
    ctx, rx, chans = slot
    dec, sub, E, n_total, n_ch = _check(ctx, chans, BIG, "exact-all")
    assert (E, n_ch) == (E0, 3)
    counts = [int((dec["ch_id"] == ch).sum()) for ch in chans]
    print("decodes per channel:", counts)
    assert counts[0] >= 2 and counts[1] == 1 and counts[2] == 0, counts          # several, one, none
    # the fits do find the transmissions: most of the footprint's energy is taken out of the decodes that are not faded copies
    print("p_removed / p_before:", np.round(sub["p_removed"] / sub["p_before"], 3))
    # the channel without a decode: the frame's own bits
    audio, _ = ctx.fetch_audio_f32(chans[2])
    assert ctx.fetch_ft4_residual(chans[2])[0].tobytes() == audio[:S.N].tobytes()
    # the device address is handed out under the same rule
    p, e = ctx.ft4_residual_device_ptr(chans[0])
    assert p and e == E
    # two calls on one epoch: the same bytes, reports and residuals
    res = [ctx.fetch_ft4_residual(ch)[0].tobytes() for ch in chans]
    again = ctx.subtract_ft4(E, BIG)
    assert again[0].tobytes() == dec.tobytes() and again[1].tobytes() == sub.tobytes() and again[2:] == (E, n_total, n_ch)
    assert [ctx.fetch_ft4_residual(ch)[0].tobytes() for ch in chans] == res


def test_truncation_by_max_and_null_outputs(slot):
    ctx, rx, chans = slot
    full = ctx.subtract_ft4(0, BIG)
    n_total = full[3]
    assert n_total >= 3
    # max = 0: nothing emitted, every residual is the frame; max = 1: the first decode alone is taken out; max beyond n_total: all of them
    got = ctx.subtract_ft4(0, 0)
    assert len(got[0]) == 0 and got[3] == n_total
    for ch in chans:
        assert ctx.fetch_ft4_residual(ch)[0].tobytes() == ctx.fetch_audio_f32(ch)[0][:S.N].tobytes()
    _check(ctx, chans, 1, "exact-1")
    _check(ctx, chans, n_total + 1, "exact-all")
    # null dec / null sub: the counts are the same, nothing is written through the null pointer, the residual is made all the same
    for null_dec, null_sub in ((True, False), (False, True), (True, True)):
        dec, sub = np.zeros(n_total, full[0].dtype), np.zeros(n_total, full[1].dtype)
        t0, n, nt, nc = C.c_uint64(0), C.c_int(-1), C.c_int(-1), C.c_int(-1)
        rc = ctx.L.cwslg_subtract_ft4(ctx.h, C.byref(t0), None if null_dec else dec.ctypes.data, None if null_sub else sub.ctypes.data, n_total,
                                      C.byref(n), C.byref(nt), C.byref(nc))
        assert (rc, t0.value, n.value, nt.value, nc.value) == (0, E0, n_total, n_total, 3)
        assert null_dec or dec.tobytes() == full[0].tobytes()
        assert null_sub or sub.tobytes() == full[1].tobytes()
        want = _REF["exact-all"][1]
        assert all(ctx.fetch_ft4_residual(ch)[0].tobytes() == want[ch].tobytes() for ch in chans)


def test_the_call_changes_nothing_else(slot):
    ctx, rx, chans = slot

    def state():
        out = [repr(sorted(ctx.stats().items()))]
        for ch in chans:
            soft = ctx.fetch_ft4_softbits(ch, 1800)
            out += [ctx.fetch_audio_f32(ch)[0].tobytes(), ctx.sync_debug(ch, "ft4_cx").tobytes(), repr(ctx.fetch_candidates(ch, 600)),
                    repr(ctx.fetch_ft4_sync(ch, 1800)), tuple(np.asarray(a).tobytes() for a in soft), ctx.fetch_ft4_decode(ch, 1800).tobytes(),
                    ctx.fetch_ft4_osd(ch, 1800).tobytes(), ctx.fetch_frame(ch)["i16"].tobytes()]
        out.append(ctx.fetch_decodes(MODE, 0, BIG)[0].tobytes())
        out.append(tuple(a.tobytes() for a in ctx.fetch_ft4_decode_reports(0, BIG)[:2]))
        return out
    before = state()
    sync_launches = ctx.stats()["sync_launches"]
    ctx.subtract_ft4(0, BIG)
    ctx.subtract_ft4(0, 1)
    assert ctx.stats()["sync_launches"] == sync_launches
    assert state() == before


def test_error_paths(slot):
    import cwsl_digi_amd as P
    ctx, rx, chans = slot
    t0, n, nt = C.c_uint64(0), C.c_int(-1), C.c_int(-1)
    assert ctx.L.cwslg_subtract_ft4(ctx.h, None, None, None, 0, C.byref(n), C.byref(nt), None) == ERR_ARG
    assert ctx.L.cwslg_subtract_ft4(ctx.h, C.byref(t0), None, None, 0, None, C.byref(nt), None) == ERR_ARG
    assert ctx.subtract_ft4(E0 + 15, BIG) is None                       # no channel has that epoch
    with pytest.raises(P.CwslGpuError) as e:
        ctx.fetch_ft4_residual(99)
    assert e.value.status == ERR_ARG
    out = np.zeros(10, np.float32)
    assert ctx.L.cwslg_fetch_ft4_residual(ctx.h, chans[0], out.ctypes.data, out.size, None, None) == ERR_ARG      # destination too small
    # the FT8 calls keep ignoring the FT4 group: no FT8 channel takes part, an FT4 channel has no FT8 residual
    assert ctx.subtract_ft8() is None and ctx.fetch_ft8_residual(chans[0]) is None
    # a table without systematic form: decodes as before, no subtraction
    with P.Context(0) as c2:
        rx2, ch2 = _open(c2, code=K.singular_table(SEED))
        _slot(c2, rx2, 0)
        assert c2.fetch_decodes(MODE) is not None
        with pytest.raises(P.CwslGpuError) as e:
            c2.subtract_ft4()
        assert e.value.status == ERR_ARG and "systematic" in str(e.value)
        assert c2.fetch_ft4_residual(ch2[0]) is None


def test_ft8_channels_have_no_ft4_subtraction():
    """the FT8 group: a context with FT8 channels alone has no FT4 channel that takes part (CWSLG_ERR_NO_FRAME), and an FT8 channel's id has no
    FT4 residual"""
    import cwsl_digi_amd as P
    with P.Context(0) as c:
        c.set_ldpc_code(LC.make_code(SEED)["nm"])
        rx = c.receiver_open(RC.FS, RC.BLK["FT8"], 0)
        ch = c.channel_open(rx, RC.RF["FT8"][0], "FT8")
        c.slot_boundary("FT8", RC.start_epoch("FT8", 0))
        t0, n, nt, nc = C.c_uint64(0), C.c_int(-1), C.c_int(-1), C.c_int(-1)
        assert c.L.cwslg_subtract_ft4(c.h, C.byref(t0), None, None, 0, C.byref(n), C.byref(nt), C.byref(nc)) == NO_FRAME
        assert (n.value, nt.value, nc.value) == (0, 0, 0)
        out = np.zeros(S.N, np.float32)
        assert c.L.cwslg_fetch_ft4_residual(c.h, ch, out.ctypes.data, out.size, None, None) == NO_FRAME
        assert c.fetch_ft4_residual(ch) is None and c.ft4_residual_device_ptr(ch) is None


def test_fast_mode_frame():
    """cwslg_set_exact(ctx, 0): the fused polyphase frame differs from the exact one in its last bits; the subtractor works on the frame that is
    there, and the same equality holds"""
    import cwsl_digi_amd as P
    with P.Context(0) as c:
        c.set_exact(False)
        rx, chans = _open(c)
        _slot(c, rx, 0)
        got = _check(c, chans, BIG, "fast-all")
        assert got[3] >= 1


SHORT_BLOCKS = 235                 # receiver blocks of the slot that ends early


def _device_floats(ctx, ptr, n):
    """n floats at a device address, through the HIP runtime the library itself is linked to"""
    out = np.empty(n, np.float32)
    ctx.synchronize()
    ctx.L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert ctx.L.hipMemcpy(out.ctypes.data, ptr, 4 * n, 2) == 0         # (2: hipMemcpyDeviceToHost)
    return out


def test_short_slot_after_two_full_ones():
    """A slot that ended early, after two full ones have left a loud full-length frame in both of the channel's device buffers: the device frame
    does not hold the zero tail, so desc.n_valid is what keeps the fit's window and the apply's frame load from the earlier slot's samples.
    The reference is the restatement on cwslg_fetch_audio_f32's frame, whose tail is +0.  n_valid lies inside the span of an emitted decode.
    The frame grows by whole receiver blocks, 256 samples each, so n_valid can only be a multiple of 4 here: the masks are reached a
    whole vector at a time."""
    import cwsl_digi_amd as P
    with P.Context(0) as c:
        rx, chans = _open(c)
        _slot(c, rx, 0)
        _slot(c, rx, 1)
        _slot(c, rx, 2, SHORT_BLOCKS)
        dec, sub, E, n_total, n_ch = _check(c, chans, BIG, "short-all")
        assert (E, n_ch) == (RC4.start_epoch(2), 3) and n_total >= 1
        nv = [c.fetch_audio_f32(ch)[1] for ch in chans]
        assert len(set(nv)) == 1 and 0 < nv[0] < S.N
        n_valid = nv[0]
        assert n_valid % 4 == 0 and n_valid == SHORT_BLOCKS * RC4.BLK * 12000 // RC4.FS
        # where the fits put the decodes: n_valid strictly inside the span of at least one
        start = np.rint(sub["dt_s"].astype(np.float64) * 12000.0).astype(np.int64) + 6000
        cut = (start < n_valid) & (n_valid < start + S.NW)
        print("short slot: n_valid", n_valid, "n_valid % 4", n_valid % 4, "decodes per channel", [int((dec["ch_id"] == ch).sum()) for ch in chans],
              "starts", start.tolist(), "cut by n_valid", cut.tolist())
        assert cut.any()
        # the device frame past n_valid is NOT zero: what the slot before the last left there
        for ch in chans:
            i16, f32 = c.frame_device_ptrs(ch)
            dev = _device_floats(c, f32, S.N)
            assert dev[:n_valid].tobytes() == c.fetch_audio_f32(ch)[0][:n_valid].tobytes()
            assert np.count_nonzero(dev[n_valid:]) > (S.N - n_valid) // 2


def _cut_references(ctx, chans, dec):
    """_REF["max-<k>"] for every k = 0 .. len(dec) + 1, as _want would make them one by one: a fit reads the original frame alone, so the fits
    are made once and the residual of a cut list is the restatement's apply over the fits that are left"""
    G = K.encoder(SEED)
    audio = {ch: ctx.fetch_audio_f32(ch)[0][:S.N] for ch in chans}
    fits = [S.fit(audio[d["ch_id"]], R4.tones(G, d["bits"]), d["freq_hz"], d["dt_s"]) for d in dec]
    sub = np.array([f[0] for f in fits], S.SUB_DTYPE).reshape(-1)
    for k in range(len(dec) + 2):
        _REF["max-%d" % k] = (sub[:k], {ch: S.apply(audio[ch], [f[1] for f, d in zip(fits[:k], dec[:k]) if d["ch_id"] == ch]) for ch in chans})


def test_every_max():
    """max = 0 .. n_total + 1: the list cut in front of the first decode, inside a channel, exactly at a channel's end (where the apply's p_lo and
    p_hi clamp against the emitted count) and not at all"""
    import cwsl_digi_amd as P
    with P.Context(0) as c:
        rx, chans = _open(c)
        _slot(c, rx, 0)
        n_total = c.subtract_ft4(0, BIG)[3]
        counts = [int((c.fetch_decodes(MODE, 0, BIG)[0]["ch_id"] == ch).sum()) for ch in chans]
        assert n_total == sum(counts) and counts[0] >= 2 and counts[1] == 1
        _cut_references(c, chans, c.fetch_decodes(MODE, 0, BIG)[0])
        for mx in range(n_total + 2):
            got = _check(c, chans, mx, "max-%d" % mx)
            assert len(got[0]) == min(mx, n_total) and got[3] == n_total
        # (max = counts[0] ends on the first channel's boundary, counts[0] + 1 is one decode into the second)
        assert counts[0] + 1 <= n_total


def test_residual_block_grows_with_the_channels():
    """The group's residual block is sized by the channels of the first call; nine more channels on the same receiver, at the first channel's
    dial offset, take part in the next slot: the block is freed and made anew, every new channel hears what channel 0 hears and gets its reports
    and its residual, byte for byte, and the first three still agree with the restatement."""
    import cwsl_digi_amd as P
    with P.Context(0) as c:
        rx, chans = _open(c)
        _slot(c, rx, 0)
        assert c.subtract_ft4(0, BIG)[4] == 3
        more = [c.channel_open(rx, RFS[0], MODE) for _ in range(9)]
        for ch in more:
            c.slot_boundary_channel(ch, RC4.start_epoch(1))                  # (a channel's first boundary starts its first slot)
        _slot(c, rx, 1)
        dec, sub, E, n_total, n_ch = c.subtract_ft4(0, BIG)
        assert (E, n_ch) == (RC4.start_epoch(1), 12) and len(dec) == n_total
        # the first three channels against the restatement
        old = np.isin(dec["ch_id"], chans)
        want_sub, want_res = _want(c, chans, dec[old], "grow-12")
        assert sub[old].tobytes() == want_sub.tobytes()
        for ch in chans:
            assert c.fetch_ft4_residual(ch)[0].tobytes() == want_res[ch].tobytes()
        # the nine new ones against channel 0
        mine = dec["ch_id"] == chans[0]
        assert mine.sum() >= 2
        a0 = c.fetch_audio_f32(chans[0])[0].tobytes()
        for ch in more:
            assert c.fetch_audio_f32(ch)[0].tobytes() == a0
            its = dec["ch_id"] == ch
            assert its.sum() == mine.sum() and dec["bits"][its].tobytes() == dec["bits"][mine].tobytes()
            assert sub[its].tobytes() == sub[mine].tobytes()
            r, e = c.fetch_ft4_residual(ch)
            assert e == E and r.tobytes() == want_res[chans[0]].tobytes()


def test_residual_is_gone_after_the_next_boundary(slot):
    """(the last test on the shared context: it moves the group on)"""
    ctx, rx, chans = slot
    ctx.subtract_ft4(0, BIG)
    assert ctx.fetch_ft4_residual(chans[0]) is not None
    _slot(ctx, rx, 1)                                                   # the frames are now of the next epoch; the block still holds slot 0
    for ch in chans:
        assert ctx.fetch_ft4_residual(ch) is None and ctx.ft4_residual_device_ptr(ch) is None
    t0 = C.c_uint64()
    out = np.zeros(S.N, np.float32)
    assert ctx.L.cwslg_fetch_ft4_residual(ctx.h, chans[0], out.ctypes.data, out.size, None, C.byref(t0)) == NO_FRAME and not out.any()
    got = ctx.subtract_ft4(0, BIG)                                      # the new slot: residuals again, of its epoch
    assert got[2] == RC4.start_epoch(1) and ctx.fetch_ft4_residual(chans[0])[1] == got[2]
