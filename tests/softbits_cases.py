"""Test helper: the signal recipes of tests/test_gpu_softbits_scale.py, vetted on the CPU by tests/test_softbits_scale_inputs.py.

Workload of every recipe: one 48 kHz receiver, blocks of 1024.  An FT4 slot is N4 = 359 424 IQ samples (360 000 rounded down to whole
blocks); a "pair slot" is N8 = 2 N4 = 718 848 samples (the FT8 slot of 720 000, rounded down to two whole FT4 slots): the FT8 group sees one
boundary at its end, the FT4 group one in the middle and one at the end, so that the FT8 frame and the SECOND FT4 frame end at one epoch.  FT4
bursts of a pair slot lie in that second half (their t0 counts from its start).

A burst is (audio_hz, t0_s, amp, tone_seed): tone 0 at the channel's dial frequency + audio_hz, first symbol t0_s into the frame, tones from
ft8_softbits_ref.ft8_iq_with_tones / ft4_softbits_ref.ft4_iq_with_tones, so the transmitted bits are known.  Noise is oracle.synth_iq scaled
by NOISE (sigma about 350 over the 48 kHz against amplitudes of 2000 and more): every burst must decode without a single wrong hard decision.

The helpers at the end state the conditions that BOTH the CPU module (on the oracle's own frames) and the GPU module (on the library's output)
assert, so a GPU test cannot pass by producing too little to compare."""
import numpy as np

import ft4_softbits_ref as R4
import ft8_softbits_ref as R8

FS, BLK = 48000, 1024
N4 = 360000 // BLK * BLK
N8 = 2 * N4
T_HALF = N4 / FS                       # start of a pair slot's second FT4 frame, seconds into the pair slot
NOISE = 0.3
U32 = np.uint32


def noise_iq(oracle, seed, n):
    return (oracle.synth_iq(seed, n, FS, tones_hz=[], amp=0.0) * NOISE).astype(np.complex64)


def build_iq(oracle, seed, n, ft8=(), ft4=(), ft4_t_off=0.0):
    """ft8 / ft4: [(dial_hz, [burst, ...])] -> (iq complex64[n], {("FT8" | "FT4", dial_hz): [tones per burst]})"""
    iq = noise_iq(oracle, seed, n).astype(np.complex128)
    tones = {}
    for f, bursts in ft8:
        tones[("FT8", f)] = []
        for a, t0, amp, ts in bursts:
            s, t = R8.ft8_iq_with_tones(FS, n, f, a, t0, amp, ts)
            iq += s
            tones[("FT8", f)].append(t)
    for f, bursts in ft4:
        tones[("FT4", f)] = []
        for a, t0, amp, ts in bursts:
            s, t = R4.ft4_iq_with_tones(FS, n, f, a, ft4_t_off + t0, amp, ts)
            iq += s
            tones[("FT4", f)].append(t)
    return iq.astype(np.complex64), tones


def pair_iq(oracle, seed, ft8=(), ft4=()):
    """One pair slot: FT8 bursts anywhere in it, FT4 bursts in its second half."""
    return build_iq(oracle, seed, N8, ft8, ft4, ft4_t_off=T_HALF)


# ---- 1. FT4 at 37 channels in one boundary -----------------------------------------------------------------------------------------------
# 37 dials 1100 Hz apart.  The 6 kHz passbands overlap: a burst of channel p at audio a also lies in channel k at a + 1100 (p - k) while that
# is inside 0..6000 Hz, i.e. for k = p - 5 .. p + 2.  The probes are therefore kept 8 and more channels apart except the adjacent pair 17 / 18,
# whose audio frequencies are chosen so that what one sees of the other (17's 2300 Hz at 1200 Hz in 18; 18's 1450 / 2400 Hz at 2550 / 3500 Hz
# in 17) is no probe's own frequency.  Channels 3 and 30 have no probe burst inside their search range (200..3000 Hz): noise only there, apart from
# the attenuated mirror image of a burst just below the dial (27's 2850 Hz shows near 390 Hz in channel 30), which is no probe's frequency either.
MANY_DIALS = [-23000 + 1100 * k for k in range(37)]
MANY_PROBES = {
    0: [(600.0, 0.50, 3000.0, 201), (1700.0, 0.85, 2600.0, 202), (2700.0, 0.30, 2800.0, 203)],
    9: [(750.0, 0.65, 3000.0, 204), (2050.0, 0.40, 2700.0, 205)],
    17: [(900.0, 0.95, 2900.0, 206), (2300.0, 0.55, 2600.0, 207)],
    18: [(1450.0, 0.35, 3000.0, 208), (2400.0, 0.75, 2700.0, 209)],
    27: [(1050.0, 0.45, 2800.0, 210), (1950.0, 1.05, 3000.0, 211), (2850.0, 0.70, 2600.0, 212)],
    36: [(500.0, 0.60, 3000.0, 213), (1600.0, 0.90, 2700.0, 214)],
}
MANY_NOISE_ONLY = [3, 30]


def many_channels_iq(oracle):
    return build_iq(oracle, 301, N4, ft4=[(MANY_DIALS[k], b) for k, b in MANY_PROBES.items()])


# ---- 2. both features, 5 FT8 + 3 FT4 channels: three pair slots -------------------------------------------------------------------------
# (dials 5500 Hz apart: a burst at audio a lies at 5500 + a in the channel below -- past every search range used here -- and not at all in the one above)
GRID = [-22000 + 5500 * k for k in range(8)]
BOTH_FT8_DIALS, BOTH_FT4_DIALS = GRID[:5], GRID[5:]


def both_slot(k):
    """-> (seed, ft8 [(dial, bursts)], ft4 [(dial, bursts)]) of pair slot k = 0, 1, 2: two FT8 bursts and two FT4 bursts per channel"""
    ft8 = [(f, [(500.0 + 187.5 * j + 62.5 * k, 0.56 + 0.08 * j, 3000.0, 400 + 10 * k + j),
                (1800.0 + 125.0 * j + 93.75 * k, 1.00 + 0.12 * j, 2500.0, 450 + 10 * k + j)]) for j, f in enumerate(BOTH_FT8_DIALS)]
    ft4 = [(f, [(700.0 + 250.0 * j + 110.0 * k, 0.40 + 0.10 * j, 3000.0, 500 + 10 * k + j),
                (2100.0 + 200.0 * j - 90.0 * k, 0.80 + 0.05 * j, 2600.0, 550 + 10 * k + j)]) for j, f in enumerate(BOTH_FT4_DIALS)]
    return 310 + k, ft8, ft4


# ---- 3. reconfiguration: one FT8 and one FT4 channel, six pair slots --------------------------------------------------------------------
RECONF_FT8_DIAL, RECONF_FT4_DIAL = -12000, 9000
# (max_cand, f_hi, order) in force at the END of pair slot k
RECONF_CONFIG = [(100, 3000, "sync"), (7, 3000, "sync"), (200, 3000, "sync"), (200, 2959, "sync"), (200, 3100, "freq"), (100, 3000, "sync")]


def reconf_slot(k):
    """Two FT8 and two FT4 probe bursts per slot, moving with k.  Slot 1 (max_cand 7) carries seven weaker bursts of each kind besides, so that
    both full lists are longer than 7 and the cut is a real one; the probes stay inside it."""
    ft8b = [(600.0 + 156.25 * k, 0.60 + 0.04 * k, 3000.0, 600 + k), (2300.0 - 125.0 * k, 1.12 - 0.08 * k, 2600.0, 610 + k)]
    ft4b = [(800.0 + 170.0 * k, 0.35 + 0.07 * k, 3000.0, 620 + k), (2800.0 - 160.0 * k, 0.90 - 0.06 * k, 2700.0, 630 + k)]
    if k == 1:
        ft8b += [(1000.0 + 112.5 * j, 0.52 + 0.16 * j, 400.0, 640 + j) for j in range(7)]
        # (getcandidates4 scans upwards and stops at max_cand BEFORE ordering: the cut keeps the seven lowest peaks, so the probes go lowest)
        ft4b = [(450.0, 0.42, 3000.0, 621), (720.0, 0.84, 2700.0, 631)] + [(1000.0 + 250.0 * j, 0.30 + 0.11 * j, 400.0, 650 + j) for j in range(7)]
    return 320 + k, [(RECONF_FT8_DIAL, ft8b)], [(RECONF_FT4_DIAL, ft4b)]


# ---- 4. channels that come and go: three pair slots --------------------------------------------------------------------------------------
CHURN_DIALS = dict(zip("ABCDPQRS", GRID))


def churn_slot(k):
    """Slot 0: A B C / P Q R.  Slot 1: B C D / Q R S.  Slot 2: B C D / no FT4 channel."""
    names8 = ["ABC", "BCD", "BCD"][k]
    names4 = ["PQR", "QRS", ""][k]
    ft8 = [(CHURN_DIALS[c], [(450.0 + 218.75 * j + 93.75 * k, 0.56 + 0.12 * j, 3000.0, 700 + 10 * k + j),
                             (1900.0 + 156.25 * j - 62.5 * k, 1.04 + 0.08 * j, 2600.0, 750 + 10 * k + j)]) for j, c in enumerate(names8)]
    ft4 = [(CHURN_DIALS[c], [(650.0 + 230.0 * j + 130.0 * k, 0.45 + 0.10 * j, 3000.0, 800 + 10 * k + j),
                             (2200.0 + 180.0 * j - 70.0 * k, 0.85 + 0.05 * j, 2700.0, 850 + 10 * k + j)]) for j, c in enumerate(names4)]
    return 330 + k, names8, names4, ft8, ft4


# ---- 5. small and large lists -----------------------------------------------------------------------------------------------------------
LISTS_FT8_DIAL, LISTS_FT4_DIAL = 4000, -15000
LISTS_FOUR = [(562.5, 0.56, 3000.0, 901), (1250.0, 0.76, 2800.0, 902), (1937.5, 0.96, 2600.0, 903), (2625.0, 1.16, 2400.0, 904)]


def dense_bursts(n):
    """n FT8 signals (12 <= n <= 16) spread over 300..2800 Hz and 0.5..1.9 s with amplitudes 600..2500, as test_candidate_order_option_and_dense_lists draws them"""
    rng = np.random.default_rng(77)
    out = []
    for j in range(n):
        a = 300.0 + 3.125 * int(rng.integers(0, 800))
        out.append((a, 0.52 + 0.04 * int(rng.integers(0, 36)), float(rng.uniform(600, 2500)), 920 + j))
    return out


LISTS_DENSE = dense_bursts(16)
LISTS_MANY8, LISTS_FEW8 = dense_bursts(12), [(1500.0, 0.72, 3000.0, 940)]
LISTS_MANY4 = [(450.0 + 420.0 * j, 0.30 + 0.12 * j, 2000.0 + 200.0 * j, 950 + j) for j in range(6)]
LISTS_FEW4 = [(1650.0, 0.55, 300.0, 960)]            # (a lone STRONG burst leaves more entries than the six: noise peaks pass the threshold beside it)

# ---- 6. the band edges: enable_sync(True, 1.5, 100, 100, 5000) ---------------------------------------------------------------------------
EDGE_DIAL = -10000
EDGE_BURSTS = [(215.0, 0.50, 3000.0, 971), (4830.0, 0.80, 3000.0, 972), (2400.0, 0.35, 2800.0, 973)]

# ---- 7. fetch_slot next to the soft fetches: one pair slot -------------------------------------------------------------------------------
TICKET_FT8 = [(RECONF_FT8_DIAL, [(812.5, 0.64, 3000.0, 981), (1687.5, 0.92, 2700.0, 982), (2437.5, 1.20, 2500.0, 983)])]
TICKET_FT4 = [(RECONF_FT4_DIAL, [(700.0, 0.40, 3000.0, 984), (1600.0, 0.75, 2800.0, 985), (2500.0, 1.00, 2600.0, 986)])]


# ---- the oracle's own chain ---------------------------------------------------------------------------------------------------------------
def oracle_frame(oracle, mode, dial_hz, iq, split=None):
    """The int16 frame of the LAST slot of `iq` by oracle.Channel: boundary, push, [boundary at `split`, push,] boundary."""
    oc = oracle.Channel(mode, FS, BLK, dial_hz)
    try:
        assert oc.boundary(1) is None
        if split:
            oc.push_many(iq[:split])
            assert oc.boundary(8) is not None
            oc.push_many(iq[split:])
        else:
            oc.push_many(iq)
        return oc.boundary(16)["i16"]
    finally:
        oc.close()


# ---- the restatement on a frame + list ----------------------------------------------------------------------------------------------------
def ft8_reference(oracle, i16, cands, pitch):
    plane = oracle.ft8_spectra(i16, pitch)
    llr, sigma, nsync = R8.softbits(plane, cands)
    return dict(plane=plane, llr=llr, sigma=sigma, nsync=nsync)


def ft4_reference(oracle, i16, cands):
    recs = oracle.ft4_sync_all(i16, cands)
    cx = oracle.ft4_bigspec(i16)
    llr, sigma, nsync, nqual = R4.softbits_of_records(oracle, cx, recs)
    return dict(recs=recs, cx=cx, llr=llr, sigma=sigma, nsync=nsync, nqual=nqual)


def key(cands):
    """A candidate list as comparable bits"""
    return [(c[0], c[1]) + tuple(int(np.float32(x).view(U32)) for x in c[2:]) for c in cands]


# ---- the conditions (asserted on the CPU for the oracle's frames and on the GPU for the library's records) ------------------------------
def ft8_best(cands, burst):
    """Index of the strongest list entry at the burst's bin whose lag is the burst's start: symbol n of entry (i, j) sits at the 1-based step
    j + 12 + 4 n, i.e. at (j + 11) 0.04 s, and dt_s = (j - 0.5) 0.04 s, so a burst that starts t0 into the frame has dt_s = t0 - 0.46 s (FT8 start times here
    are whole steps; within 0.03 s)"""
    want = int(round(burst[0] / 3.125))
    near = [q for q, c in enumerate(cands) if c[0] == want and abs(c[4] - (burst[1] - 0.46)) <= 0.03]
    assert near, ("burst not in the list", burst[:2], [c for c in cands if abs(c[0] - want) <= 2][:5])
    return max(near, key=lambda q: cands[q][2])


def assert_ft8_found(cands, llr, nsync, bursts, tones):
    for b, tn in zip(bursts, tones):
        q = ft8_best(cands, b)
        bits = R8.tone_bits(tn) == 1
        assert nsync[q] == 21 and np.array_equal(llr[q] > 0, bits), (b[:2], int(nsync[q]), int(((llr[q] > 0) != bits).sum()))


def ft4_best(recs, burst):
    near = [q for q, h in enumerate(recs) if abs(h["f1_hz"] - burst[0]) <= 2.0 and abs(h["ibest"] / 666.67 - burst[1]) <= 0.006]
    assert near, ("burst not among the records", burst[:2], [(h["f1_hz"], h["ibest"]) for h in recs if abs(h["f1_hz"] - burst[0]) <= 30.0][:5])
    return max(near, key=lambda q: recs[q]["sync"])


def assert_ft4_found(recs, llr, nsync, bursts, tones):
    for b, tn in zip(bursts, tones):
        q = ft4_best(recs, b)
        bits = R4.tone_bits(tn) == 1
        assert nsync[q] == 16 and np.array_equal(llr[q, 0] > 0, bits), (b[:2], int(nsync[q]), int(((llr[q, 0] > 0) != bits).sum()))


def assert_no_foreign_record(recs, own_probe, probes=None):
    """No strong record (sync > 2.5) of this probe channel at another probe's audio frequency"""
    probes = MANY_PROBES if probes is None else probes
    for p, bursts in probes.items():
        if p == own_probe:
            continue
        for b in bursts:
            hit = [h for h in recs if abs(h["f1_hz"] - b[0]) <= 2.0 and h["sync"] > 2.5]
            assert not hit, (own_probe, p, b[0], hit[:2])
