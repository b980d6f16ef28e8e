"""Test helper: the recipes of tests/test_gpu_longsync_edges.py, vetted on the CPU by tests/test_longsync_cases_inputs.py.

Sizes.  One 48 kHz receiver, blocks of 2048, 703 blocks (30 s, 1 439 744 complex samples) per S120 slot.  Both searches read the whole 120 s
frame, zero tail included, whatever the slot held, and neither ever sees the IQ rate: a quarter of the time at a quarter of the rate is
a sixteenth of the demodulation and the same search.

Receiver A.  One composite IQ, the same in every slot, with four WSPR and five FST4W-120 channels on it, opened in the interleaved order
of A_CHANNELS so that a channel's place in its mode's batched launch is not its place in the context.  The noise is oracle.synth_iq passed
through a mask over frequency (FFT, gain, inverse FFT), because nine 6 kHz passbands do not fit into 48 kHz side by side and two channels
are to hear no noise at all:
    -24000 .. 1500 Hz    flat noise: the four noisy FST4W channels (dials 6500 Hz apart, searched up to 4800 Hz of audio)
      1500 .. 8500 Hz    nothing: the FST4W channel at 2000 Hz hears only its carrier
      8500 .. 17200 Hz   flat noise: three WSPR channels, whose searches look at 1500 +- 150 Hz of audio only; around 15500 Hz (the band of
                         the noise-only WSPR channel) the gain ripples with a period of 37 Hz -- flat noise never reaches wsprd's -8 dB
                         floor (oracle: 0 candidates), and an empty list compares equal to anything
     17200 .. 24000 Hz   nothing: the WSPR channel at 18000 Hz hears only its carrier
The +-110 Hz edge of wsprd's list.  Bin j of the 512-point half-symbol spectra is 1500 Hz + j * 0.732421875 Hz exactly; +-150 is 109.86 Hz
(kept), +-151 is 110.60 Hz (dropped).  smspec is a 7-bin running sum, so two carriers in adjacent bins make ONE plateau whose maximum the noise
places; a carrier alone on a bin centre makes a strict maximum AT its bin (the sine window's side lobes fall off as 1 / (1 - 4 k^2): the
sum centred on the carrier gains the lobe at distance 3 and loses the one at 4, on both sides).  So each side of 1500 Hz carries ONE edge
carrier per channel: `W_carriers` has +150 (kept) and -151 (dropped) and one mid-band carrier, `W_tx` has -150 (kept) and +151 (dropped)
next to its transmission.  Between them every comparison of the filter sees a peak on each side of it.

Receiver B.  All-zero IQ, one WSPR and one FST4W-120 channel: int16 frames of zeros (factor = 32767 / (0 + 1)).

Window walk.  WALK[k] = (nfa_hz, nfb_hz, minsync) is in force at the END of slot k (slot k runs from epoch 120 (k + 1))."""
import numpy as np

import longsync_signal as LS

FS, BLK, NBLK = 48000, 2048, 703
N = BLK * NBLK
DFW = 375.0 / 512.0                      # wsprd's bin: 0.732421875 Hz
U32 = np.uint32

# name, mode, dial (Hz from the LO), in the order the GPU test opens them
A_CHANNELS = [
    ("F_fsk1500", "FST4W-120", -24000),
    ("W_carriers", "WSPR", 9000),
    ("F_fsk150", "FST4W-120", -17500),
    ("W_tx", "WSPR", 11500),
    ("F_fsk4750", "FST4W-120", -11000),
    ("F_noise", "FST4W-120", -4500),
    ("W_noise", "WSPR", 14000),
    ("F_carrier", "FST4W-120", 2000),
    ("W_carrier", "WSPR", 18000),
]
B_CHANNELS = [("W_zero", "WSPR", 3000), ("F_zero", "FST4W-120", -9000)]
DIAL = {n: d for n, _, d in A_CHANNELS + B_CHANNELS}
MODE = {n: m for n, m, _ in A_CHANNELS + B_CHANNELS}
A_WSPR = [n for n, m, _ in A_CHANNELS if m == "WSPR"]
A_FST = [n for n, m, _ in A_CHANNELS if m != "WSPR"]
assert len(A_WSPR) == 4 and len(A_FST) == 5

NOISE_SEED, TONE_SEED = 1201, 1202
NOISE_BANDS = [(-24000.0, 1500.0), (8500.0, 17200.0)]
RIPPLE_AT, RIPPLE_HALF, RIPPLE_PERIOD, RIPPLE_DEPTH = 15500.0, 200.0, 37.0, 0.6
# (channel, audio Hz, amplitude): steady carriers.  synth_iq's noise has sigma 1182 per component over the 48 kHz.
CARRIERS = [
    ("W_carriers", 1500.0 + 150 * DFW, 3000.0), ("W_carriers", 1500.0 - 151 * DFW, 3000.0), ("W_carriers", 1500.0 + 41 * DFW, 2000.0),
    ("W_tx", 1500.0 - 150 * DFW, 3000.0), ("W_tx", 1500.0 + 151 * DFW, 3000.0),
    ("W_carrier", 1500.0 + 20 * DFW, 6000.0),
    ("F_carrier", 1500.0, 6000.0),
]
WSPR_TX = ("W_tx", 1500.0 + 41.0, 2.0, 1500.0)                   # tone 0 at audio Hz, start s, amplitude
FSK = [("F_fsk1500", 1500.0, 1.0, 1500.0), ("F_fsk1500", 1451.0, 0.4, 800.0), ("F_fsk150", 150.0, 1.0, 1500.0), ("F_fsk4750", 4750.0, 1.0, 1500.0)]

WALK = [
    (1400, 1600, 1.2),
    (100, 300, 0.5),
    (50, 250, 0.5),         # nfa clamps to 100
    (4600, 4800, 0.5),
    (4700, 4900, 0.5),      # nfb clamps to 4800
    (1400, 1607, 0.1),      # the widest window the band table holds (200 entries per residue), and the list cap of 100
    (1500, 1506, 1.2),      # npts 3
    (1500, 1505, 1.2),      # npts 2
    (1500, 1500, 1.2),      # npts < 1: no percentile, no list
    (1400, 1600, 1.2),
]
DEFAULT_WINDOW = WALK[0]
REJECTED_WINDOW = (1400, 1608)

_cache = {}


def receiver_a_iq(oracle):
    """complex64[N]: the composite of receiver A"""
    if "a" in _cache:
        return _cache["a"]
    f = np.fft.fftfreq(N, 1.0 / FS)
    gain = np.zeros(N)
    for lo, hi in NOISE_BANDS:
        gain[(f >= lo) & (f <= hi)] = 1.0
    rip = np.abs(f - RIPPLE_AT) <= RIPPLE_HALF
    gain[rip] = 1.0 + RIPPLE_DEPTH * np.cos(2.0 * np.pi * (f[rip] - RIPPLE_AT) / RIPPLE_PERIOD)
    noise = oracle.synth_iq(NOISE_SEED, N, FS, tones_hz=[], amp=0.0).astype(np.complex128)
    iq = np.fft.ifft(np.fft.fft(noise) * gain)
    t = np.arange(N) / FS
    for name, audio, amp in CARRIERS:
        iq += amp * np.exp(2j * np.pi * (DIAL[name] + audio) * t)
    rng = np.random.default_rng(TONE_SEED)
    name, audio, t0, amp = WSPR_TX
    iq += LS.wspr_iq(FS, N, DIAL[name], audio, t0, amp, rng)
    for name, audio, t0, amp in FSK:
        iq += LS.fst4w_iq(FS, N, DIAL[name], audio, t0, amp, rng)
    _cache["a"] = iq.astype(np.complex64)
    return _cache["a"]


def receiver_b_iq():
    return np.zeros(N, np.complex64)


def oracle_frame(oracle, name, iq):
    """The int16 frame of one slot of `iq` on channel `name` by oracle.Channel: boundary, push, boundary."""
    oc = oracle.Channel(MODE[name], FS, BLK, DIAL[name])
    try:
        assert oc.boundary(120) is None
        oc.push_many(iq)
        return oc.boundary(240)["i16"]
    finally:
        oc.close()


# ---- get_candidates_fst4's derived integers and the limits of the GPU's band table, restated in float32 numpy --------------------------
def _lround(x):
    return int(np.floor(np.float64(x) + 0.5))          # positive arguments only


def fst4w_window(nfa_hz, nfb_hz, table_limits=True):
    """-> None where the library must refuse the window, else dict(ina, inb, jlo, nband, npts).  table_limits=False: get_candidates_fst4's own
    bounds only, without the two limits of the GPU's band table"""
    f32 = np.float32
    fs = f32(12000.0)
    df1, baud = fs / f32(1440000), fs / f32(8200)
    df2 = baud / f32(2.0)
    ndh = int(df2 / df1) // 2
    ina = _lround(max(f32(100.0), f32(nfa_hz)) / df2)
    inb = _lround(min(f32(4800.0), f32(nfb_hz)) / df2)
    nnw = _lround(f32(48000.0) * f32(8200) * f32(2.0) / fs)
    if inb < ina or inb >= nnw or nnw > 65600:
        return None
    jlo = _lround(f32(ina) * df2 / df1) - ndh
    jhi = _lround(f32(inb) * df2 / df1) + ndh
    nband = jhi - jlo + 1
    if jlo < 0 or jhi > 720000 or nband > 32000 or inb - ina + 9 > 1024:
        return None
    if table_limits and ((nband + 124) // 125 > 200 or jlo <= 125):     # the band table: 200 entries per residue mod 125, first entry computed for jlo > 125
        return None
    npts = min(inb, nnw - 3) - max(ina, 4) + 1 - 6
    return dict(ina=ina, inb=inb, jlo=jlo, nband=nband, npts=npts)


# ---- comparisons ------------------------------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(U32)


def same_or_both_nan(a, b):
    """float32 arrays: equal bits, or NaN on both sides (0/0 has another sign and payload on x86 than on the GPU; nothing else is allowed)"""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return a.shape == b.shape and bool(np.all((a.view(U32) == b.view(U32)) | (np.isnan(a) & np.isnan(b))))


def assert_fst4w_lists_equal(got, ref):
    assert len(got) == len(ref), (len(got), len(ref), got[:3], ref[:3])
    for q, (a, b) in enumerate(zip(got, ref)):
        assert a[2] == b[2] and bits(a[0]) == bits(b[0]), (q, a, b)
        assert same_or_both_nan(a[1], b[1]), (q, a, b)


def assert_wspr_lists_equal(got, ref):
    assert len(got) == len(ref), (len(got), len(ref))
    for q, (a, b) in enumerate(zip(got, ref)):
        assert np.array_equal(bits(a[:4]), bits(b[:4])) and a[4] == b[4], (q, a, b)


def smspec_peaks(smspec):
    """wsprd's strict local maxima, as bins relative to 1500 Hz"""
    s = np.asarray(smspec)
    j = np.arange(1, 410)
    return [int(x) - 205 for x in j[(s[j] > s[j - 1]) & (s[j] > s[j + 1])]]
