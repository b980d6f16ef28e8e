"""GPU: the 120 s candidate search at the limits of its FST4W window and on degenerate frames (recipes: tests/longsync_cases.py, vetted on
the CPU by tests/test_longsync_cases_inputs.py).  A plain exact-mode Context; the stage is fed the int16 frame in either mode.

Everything is compared on bits with oracle.wspr_search / oracle.fst4w_candidates, called with the slot's own window and fed the GPU's int16
frame.  One allowance: where the restatement's value is NaN the GPU's must be NaN too, of any sign and payload (0/0 is 0xFFC00000 on x86 and
0x7FC00000 on the GPU); bin, frequency and list length are never excused.

One context runs the ten windows of longsync_cases.WALK, one per S120 slot, on eleven channels of two receivers (`walk` below): every FST4W
channel is fetched in every slot, the WSPR channels in the first and the last.  The second table limit of the library's window check
(jlo > 125) cannot be reached from outside: the 100 Hz clamp keeps jlo at 11986 (test_longsync_cases_inputs.py::test_window_limits_restated),
so only the first (200 table entries per residue: 1400..1608 Hz) has a rejection test."""
import numpy as np
import pytest

import longsync_cases as L

pytestmark = pytest.mark.gpu
PIECE = 37 * L.BLK                                                     # 703 = 19 x 37 blocks


def _push_slot(ctx, rxs_iqs):
    for k in range(0, L.N, PIECE):
        for rx, iq in rxs_iqs:
            ctx.push_iq(rx, iq[k:k + PIECE])


@pytest.fixture(scope="module")
def walk(oracle):
    """-> dict(frames {name: int16}, slots [ {name: dict(...)} per slot ], cut7, cut1).  Nothing is compared here except that a channel's frame is the
    same in every slot (same IQ, the demodulator restarts at a boundary): one frame per channel then serves all ten windows."""
    import cwsl_digi_amd as P
    iq_a, iq_b = L.receiver_a_iq(oracle), L.receiver_b_iq()
    out = dict(frames={}, slots=[])
    with P.Context(0) as ctx:
        ctx.enable_long_sync(True, *L.WALK[0])
        rxa, rxb = ctx.receiver_open(L.FS, L.BLK, 0), ctx.receiver_open(L.FS, L.BLK, 0)
        ch = {}
        for name, mode, dial in L.A_CHANNELS[:4]:
            ch[name] = ctx.channel_open(rxa, dial, mode)
        for name, mode, dial in L.B_CHANNELS:
            ch[name] = ctx.channel_open(rxb, dial, mode)
        for name, mode, dial in L.A_CHANNELS[4:]:
            ch[name] = ctx.channel_open(rxa, dial, mode)
        ctx.slot_boundary("S120", 120)
        assert ctx.fetch_fst4w_candidates(ch["F_zero"]) is None
        for k, win in enumerate(L.WALK):
            ctx.enable_long_sync(True, *win)                           # in force at the boundary that ends the slot
            _push_slot(ctx, ((rxa, iq_a), (rxb, iq_b)))
            ctx.slot_boundary("S120", 120 * (k + 2))
            got = {}
            for name, c in ch.items():
                wspr = L.MODE[name] == "WSPR"
                if wspr and k not in (0, len(L.WALK) - 1):
                    continue
                fr = ctx.fetch_frame(c)
                assert fr["t_start"] == 120 * (k + 1) and fr["n_valid"] == L.N // 4
                if k == 0:
                    out["frames"][name] = fr["i16"].copy()
                else:
                    assert np.array_equal(fr["i16"], out["frames"][name]), (name, k)
                if wspr:
                    cands, epoch = ctx.fetch_wspr_candidates(c, with_epoch=True)
                    got[name] = dict(cands=cands, epoch=epoch, iq=ctx.long_sync_debug(c, "iq").copy(), ps=ctx.long_sync_debug(c, "ps").copy(),
                                     smspec=ctx.long_sync_debug(c, "smspec").copy())
                else:
                    cands, epoch = ctx.fetch_fst4w_candidates(c, with_epoch=True)
                    got[name] = dict(cands=cands, epoch=epoch, band=ctx.long_sync_debug(c, "band").copy(), s2=ctx.long_sync_debug(c, "s2").copy())
            if k == 0:
                out["cut1"] = {n: ctx.fetch_wspr_candidates(ch[n], max_cand=1) for n in L.A_WSPR + ["W_zero"]}
            if k == 5:
                out["cut7"] = {n: ctx.fetch_fst4w_candidates(ch[n], max_cand=7) for n in L.A_FST + ["F_zero"]}
            out["slots"].append(got)
    return out


_ref = {}


def _fst_ref(oracle, walk, name, win):
    if (name, win) not in _ref:
        _ref[(name, win)] = oracle.fst4w_candidates(walk["frames"][name], win[0], win[1], win[2], want_arrays=True)
    return _ref[(name, win)]


def _wspr_ref(oracle, walk, name):
    if name not in _ref:
        _ref[name] = oracle.wspr_search(walk["frames"][name], want_arrays=True)
    return _ref[name]


FST_ALL = L.A_FST + ["F_zero"]
WSPR_ALL = L.A_WSPR + ["W_zero"]


@pytest.mark.parametrize("k", range(len(L.WALK)))
def test_window_walk(oracle, walk, k):
    """Slot k, every FST4W channel of both receivers: band power, s2, the list and its start epoch under window WALK[k]."""
    win = L.WALK[k]
    w = L.fst4w_window(win[0], win[1])
    n_rec = []
    for name in FST_ALL:
        g = walk["slots"][k][name]
        ref, arr = _fst_ref(oracle, walk, name, win)
        assert g["epoch"] == 120 * (k + 1), name
        assert len(g["band"]) == w["nband"], (name, len(g["band"]))
        power = g["band"].real.astype(np.float32) ** 2 + g["band"].imag.astype(np.float32) ** 2           # float32, un-fused: as the oracle's band_o
        assert np.array_equal(L.bits(power), L.bits(arr["band"][:w["nband"]])), name
        if w["npts"] >= 1:                                            # below 1 the kernel returns before writing s2 and the oracle before filling it
            n = len(arr["s2"])
            assert L.same_or_both_nan(g["s2"][:n], arr["s2"]), name
            assert w["inb"] + 4 < n                                   # past the window every entry is 0 / base: zero, or NaN where base is 0
            assert np.isnan(g["s2"][n:]).all() if np.isnan(arr["s2"][-1]) else not g["s2"][n:].any(), name
        L.assert_fst4w_lists_equal(g["cands"], ref)
        n_rec.append(len(ref))
    # what the recipes promise for this slot (shown on the CPU; here on the GPU's frames)
    if k in (0, len(L.WALK) - 1):
        assert min(n_rec[:-1]) >= 1
    if win[2] == 0.1:
        assert max(n_rec) == 100
    if w["npts"] < 1:
        assert n_rec == [0] * len(n_rec)


def test_zero_frame(oracle, walk):
    """All-zero int16 frames: base = 0 and s2 = 0/0 across the window.  The restatement's scan never lets a NaN replace its pick and never
    replaces a NaN at ia: exactly one record (ia, NaN) in every window with npts >= 1; wsprd's front end sees its stray header sample as a
    single impulse and lists candidates from a nearly flat smspec."""
    for k, win in enumerate(L.WALK):
        w = L.fst4w_window(win[0], win[1])
        got = walk["slots"][k]["F_zero"]["cands"]
        if w["npts"] < 1:
            assert got == []
            continue
        assert len(got) == 1 and got[0][2] == w["ina"] and np.isnan(got[0][1]), (k, len(got), got[:3])
        assert L.bits(got[0][0]) == L.bits(_fst_ref(oracle, walk, "F_zero", win)[0][0][0])
    assert not walk["frames"]["F_zero"].any() and not walk["frames"]["W_zero"].any()
    assert len(walk["slots"][0]["W_zero"]["cands"]) >= 10


@pytest.mark.parametrize("name", WSPR_ALL)
def test_wspr_stages(oracle, walk, name):
    """iq, ps, smspec and the list of every WSPR channel, the zero-IQ one and the noiseless carrier included"""
    ref, arr = _wspr_ref(oracle, walk, name)
    for k in (0, len(L.WALK) - 1):
        g = walk["slots"][k][name]
        assert g["epoch"] == 120 * (k + 1)
        assert np.array_equal(L.bits(g["iq"].real), L.bits(arr["idat"])) and np.array_equal(L.bits(g["iq"].imag), L.bits(arr["qdat"]))
        assert np.array_equal(L.bits(g["ps"]), L.bits(arr["ps"]))
        assert np.array_equal(L.bits(g["smspec"]), L.bits(arr["smspec"]))
        L.assert_wspr_lists_equal(g["cands"], ref)
    assert len(ref) >= 1
    if name in ("W_carriers", "W_tx"):                                 # the +-110 Hz edge, on the GPU's own smspec
        kept, dropped = (150, -151) if name == "W_carriers" else (-150, 151)
        peaks = L.smspec_peaks(walk["slots"][0][name]["smspec"])
        assert kept in peaks and dropped in peaks
        assert len(walk["slots"][0][name]["cands"]) == len([p for p in peaks if abs(p) <= 150])


def test_last_slot_equals_first(walk):
    """The window is back at 1400..1600 / 1.2 after nine others: the band table was rebuilt and restored, everything equals slot 0 bit for bit."""
    a, b = walk["slots"][0], walk["slots"][-1]
    assert sorted(a) == sorted(b) == sorted(FST_ALL + WSPR_ALL)
    for name in FST_ALL:
        assert np.array_equal(a[name]["band"].view(np.uint32), b[name]["band"].view(np.uint32)), name
        assert np.array_equal(L.bits(a[name]["s2"]), L.bits(b[name]["s2"])), name
        assert len(a[name]["cands"]) == len(b[name]["cands"])
        assert [(L.bits(c[:2]).tolist(), c[2]) for c in a[name]["cands"]] == [(L.bits(c[:2]).tolist(), c[2]) for c in b[name]["cands"]], name
    for name in WSPR_ALL:
        assert [(L.bits(c[:4]).tolist(), c[4]) for c in a[name]["cands"]] == [(L.bits(c[:4]).tolist(), c[4]) for c in b[name]["cands"]], name


def test_truncated_fetches(walk):
    """max_cand below the list's length returns the list's head"""
    full = {n: walk["slots"][5][n]["cands"] for n in FST_ALL}
    assert max(len(v) for v in full.values()) == 100
    for n in FST_ALL:
        cut = walk["cut7"][n]
        assert len(cut) == min(7, len(full[n]))
        assert [(L.bits(c[:2]).tolist(), c[2]) for c in cut] == [(L.bits(c[:2]).tolist(), c[2]) for c in full[n][:7]], n
    for n in WSPR_ALL:
        cut, whole = walk["cut1"][n], walk["slots"][0][n]["cands"]
        assert len(cut) == 1 and (L.bits(cut[0][:4]).tolist(), cut[0][4]) == (L.bits(whole[0][:4]).tolist(), whole[0][4]), n


def test_rejected_window(oracle, walk):
    """A window that the band table cannot hold is refused AT enable_long_sync, like every other bad window; the previous one stays in force
    and the slot boundaries after it succeed.  (Accepted there, it failed inside slot_boundary, after the frames were finalised.)"""
    import cwsl_digi_amd as P
    prev = (100, 300, 0.5)
    iq_a = L.receiver_a_iq(oracle)
    names = ["F_fsk150", "F_noise"]
    with P.Context(0) as ctx:
        for nfa, nfb in [(1400, 1607), (1400, 1608), (1399, 1607), (100, 307), (100, 308), (4593, 4800), (4592, 4800), (1600, 1400), (100, 4800),
                         (1500, 1500), (-5, 200)]:
            if L.fst4w_window(nfa, nfb) is None:
                with pytest.raises(P.CwslGpuError):
                    ctx.enable_long_sync(True, nfa, nfb)
            else:
                ctx.enable_long_sync(True, nfa, nfb)
        ctx.enable_long_sync(True, *prev)
        rx = ctx.receiver_open(L.FS, L.BLK, 0)
        ch = {n: ctx.channel_open(rx, L.DIAL[n], L.MODE[n]) for n in names}
        ctx.slot_boundary("S120", 120)
        with pytest.raises(P.CwslGpuError):
            ctx.enable_long_sync(True, *L.REJECTED_WINDOW)
        for k in (0, 1):
            _push_slot(ctx, ((rx, iq_a),))
            ctx.slot_boundary("S120", 120 * (k + 2))
            for n in names:
                assert np.array_equal(ctx.fetch_frame(ch[n])["i16"], walk["frames"][n])
                got, epoch = ctx.fetch_fst4w_candidates(ch[n], with_epoch=True)
                ref = _fst_ref(oracle, walk, n, prev)[0]
                assert epoch == 120 * (k + 1) and len(ref) >= 1
                L.assert_fst4w_lists_equal(got, ref)
