"""Test helper: the FT8 slots of tests/test_gpu_decode_reports.py and, computed on the CPU alone, what cwslg_fetch_decode_reports must hand out for
them: tests/harvest_cases.py's machinery (oracle.Channel -> the restatements of every stage -> decodes_ref) followed by
tests/decode_reports_ref.py on the oracle's own plane.

Two channels on one 48 kHz receiver, three slots.  Channel 0 hears harvest_cases' transmissions of the slot (three strong ones, of which two sit
off the grid and come back on more than one list entry, and a weak one belief propagation fails on) and three more: one that starts so late that
its last symbols fall beyond step 372, one that started before the slot so that its first symbols fall before step 1, and one at the upper edge
of the search band; and a strong one with a SHADOW -- a second carrier of 0.7 times its amplitude that sits at tone (t + 4) mod 7 of every
symbol, exactly where the report takes its noise: the word still decodes, xsig / xnoise falls to about 2 and the report is clamped at -24 dB
(nothing weak enough for that is decoded by either decoder).  Channel 1 hears noise.  tests/test_decode_reports_inputs.py proves what the slots contain."""
import functools

import numpy as np

import decode_reports_ref as RR
import decodes_ref as DR
import ft8_softbits_ref as S8
import harvest_cases as H
import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O
import record_race_cases as RC
import report_kernel_cases as K

SEED = H.SEED
FS, BLK, RF = H.FS, H.BLK["FT8"], H.RF["FT8"]
N_EPOCHS = 3
SYNC8 = H.SYNC8
MAX_CAND = 100
LATE_STEPS, EARLY_STEPS = 66, -8                                        # start of the late / early transmission in search steps (40 ms) from the slot's start
EDGE_BIN = 958                                                          # tone 0 of the transmission at the band's upper edge (f_hi = 3000 Hz is bin 960)
EXTRA_MSEED = 900
SHADOW_BIN, SHADOW_AMP = 400, 0.7                                       # the shadowed transmission: tone 0 at this bin; the shadow's amplitude relative to it


def start_epoch(e):
    return H.start_epoch("FT8", e)


def extra_transmissions(e):
    """[(audio Hz of tone 0, start s -- may be negative, amplitude, message seed)] this module adds to harvest_cases' of slot e."""
    m = EXTRA_MSEED + 10 * e
    return [(3.125 * 300, 0.04 * LATE_STEPS, H.AMP, m), (3.125 * 600, 0.04 * EARLY_STEPS, H.AMP, m + 1), (3.125 * EDGE_BIN, 0.04 * (H.FT8_L[e] + 1), H.AMP, m + 2),
            (3.125 * SHADOW_BIN, 0.04 * (H.FT8_L[e] + 3), H.AMP, m + 3)]


def shadowed_transmission(e):
    return extra_transmissions(e)[3]


def transmissions(e):
    return H.transmissions8(e) + extra_transmissions(e)


def sent_tones(mseed):
    return C.tones_of(C.encode(SEED, C.chain_message(mseed)))


def _iq_of_tones(n, rf_hz, audio_hz, t0_s, amp, tones):
    """ldpc_cases.iq_of_tones for a start that may lie before the slot: the samples before sample 0 and after sample n are cut off."""
    sps = int(round(FS * 0.16))
    f = rf_hz + audio_hz + 6.25 * np.repeat(np.asarray(tones), sps)
    sig = amp * np.exp(1j * 2 * np.pi * np.cumsum(f) / FS)
    out = np.zeros(n, np.complex64)
    i0 = int(round(t0_s * FS))
    a, b = max(i0, 0), min(i0 + len(sig), n)
    out[a:b] = sig[a - i0:b - i0]
    return out


@functools.lru_cache(maxsize=None)
def slot_iq(e):
    """One slot of IQ (complex64, read-only): harvest_cases' slot e with the extra transmissions added."""
    iq = np.array(H.slot_iq("FT8", e), np.complex64)
    for audio, t0, amp, mseed in extra_transmissions(e):
        iq = iq + _iq_of_tones(len(iq), RF[0], audio, t0, amp, sent_tones(mseed))
    audio, t0, amp, mseed = shadowed_transmission(e)
    iq = iq + _iq_of_tones(len(iq), RF[0], audio, t0, SHADOW_AMP * amp, (sent_tones(mseed) + 4) % 7)
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def frames(k):
    from oracle import oracle as orc
    oc = orc.Channel("FT8", FS, BLK, RF[k])
    assert oc.boundary(start_epoch(0)) is None
    out = []
    for e in range(N_EPOCHS):
        oc.push_many(slot_iq(e))
        r = oc.boundary(start_epoch(e + 1))
        assert r is not None and r["t_start"] == start_epoch(e)
        out.append(r["i16"])
    oc.close()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def chain(k, e, max_cand=MAX_CAND):
    """Every stage of channel k in slot e on the CPU, the plane included."""
    from oracle import oracle as orc
    fr = frames(k)[e]
    code, G = C.make_code(SEED)["code"], OC.generator(SEED)
    cands = orc.ft8_sync(fr, SYNC8["f_lo"], SYNC8["f_hi"], SYNC8["syncmin"], max_cand)
    plane = np.ascontiguousarray(orc.ft8_spectra(fr, S8.soft_pitch(SYNC8["f_hi"])), np.float32)
    llr, sigma, nsync = S8.softbits(plane, cands)
    msg = R.hard_records(code, llr, RC.DECODE8[0], nsync, sigma, RC.DECODE8[1])
    osd = O.chain_records(G, llr, RC.OSD8[0], nsync, msg, RC.OSD8[1])
    return dict(frame=fr, plane=plane, list=cands, soft=(llr, sigma, nsync), msg=msg, osd=osd)


@functools.lru_cache(maxsize=None)
def expected(e, osd=True, max_cand=MAX_CAND):
    """(decodes, reports) of slot e with channel k under the id k."""
    cs = [chain(k, e, max_cand) for k in range(len(RF))]
    dec, _ = DR.decodes("FT8", [(k, DR.where_ft8(c["list"]), c["msg"], c["osd"] if osd else None) for k, c in enumerate(cs)])
    rep = RR.reports(K.encoder(SEED), {k: c["plane"] for k, c in enumerate(cs)}, {k: c["list"] for k, c in enumerate(cs)}, dec)
    return dec, rep


# ---- the physics of the restatement: on-grid transmissions in white noise -----------------------------------------------------------------------------
PHYS_AMPS = (1250.0, 2500.0, 5000.0, 10000.0)                           # four injected levels 6.02 dB apart, one slot each
PHYS_BINS = (200, 400, 600, 800)                                        # tone 0 of the four transmissions of a slot: on the 3.125 Hz grid
PHYS_STEP = 12                                                          # their start in search steps: on the 40 ms grid
PHYS_SIGMA = RC.SIGMA["FT8"]                                            # per component of the complex noise at FS
PHYS_NOISE_SEED, PHYS_MSEED = 77, 700


def injected_snr_db(amp):
    """SNR in 2500 Hz of a complex carrier of amplitude amp in complex white noise of PHYS_SIGMA per component at FS samples per second."""
    return 10.0 * np.log10(amp ** 2 / (2.0 * PHYS_SIGMA ** 2 * 2500.0 / FS))


@functools.lru_cache(maxsize=None)
def physics():
    """-> [(level index, bin, injected dB, reported dB, nsymerr)]: the restatement's report at the transmissions' own grid positions (the list entry
    of the oracle's search at that bin) with the tones that were sent."""
    from oracle import oracle as orc
    n = RC.N_IQ["FT8"]
    oc = orc.Channel("FT8", FS, BLK, RF[0])
    assert oc.boundary(start_epoch(0)) is None
    out = []
    for lv, amp in enumerate(PHYS_AMPS):
        rng = np.random.default_rng(PHYS_NOISE_SEED + lv)
        iq = (rng.normal(0.0, PHYS_SIGMA, n) + 1j * rng.normal(0.0, PHYS_SIGMA, n)).astype(np.complex64)
        for q, b in enumerate(PHYS_BINS):
            iq = iq + _iq_of_tones(n, RF[0], 3.125 * b, 0.04 * PHYS_STEP, amp, sent_tones(PHYS_MSEED + q))
        oc.push_many(iq.astype(np.complex64))
        fr = oc.boundary(start_epoch(lv + 1))["i16"]
        plane = np.ascontiguousarray(orc.ft8_spectra(fr, S8.soft_pitch(SYNC8["f_hi"])), np.float32)
        cands = orc.ft8_sync(fr, SYNC8["f_lo"], SYNC8["f_hi"], SYNC8["syncmin"], MAX_CAND)
        for q, b in enumerate(PHYS_BINS):
            at = [c for c in cands if c[0] == b]
            assert at, (lv, b)
            r = RR.report(plane, at[0][0], at[0][1], sent_tones(PHYS_MSEED + q))
            out.append((lv, b, float(injected_snr_db(amp)), float(r["snr_db"]), int(r["nsymerr"])))
    oc.close()
    return tuple(out)
