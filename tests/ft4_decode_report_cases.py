"""Test helper: the FT4 slots of tests/test_gpu_ft4_decode_reports.py and, computed on the CPU alone, what cwslg_fetch_ft4_decode_reports must hand
out for them: tests/harvest_twin_cases.py's machinery (oracle.Channel -> the restatements of every stage -> decodes_ref) followed by
tests/ft4_decode_reports_ref.py on the oracle's own frame spectrum.

Two channels on one 48 kHz receiver, two slots, ft4_decode_cases' / ft4_osd_cases' settings as record_race_cases applies them.  Channel 0 hears
harvest_twin_cases' transmissions of the slot (one message at two or three audio frequencies: ndup > 1; loud faded copies that only OSD returns, on
smaller entries than the copies belief propagation decodes) and three more: one that began before the frame, so that its record has ibest < 0 and its
first symbols read as +0; one that starts so late that its last symbols fall beyond baseband sample 4031; and one with a SHADOW -- a second carrier
of SHADOW_AMP times its amplitude at tone (t + 2) & 3 of every symbol, exactly where the report takes its noise, so that xsig / xnoise falls
below 1.955 and the report sits on the -21 dB floor while the word still decodes.  Channel 1 hears noise.
tests/test_ft4_decode_reports_inputs.py proves what the slots contain."""
import functools

import numpy as np

import decodes_ref as DR
import ft4_decode_cases as D
import ft4_decode_reports_ref as R4
import ft4_osd_cases as X
import ft4_softbits_ref as S4
import harvest_twin_cases as T
import ldpc_cases as C
import osd_cases as OC
import record_race_cases as RC
import report_kernel_cases as K

MODE = "FT4"
SEED = T.SEED
FS, BLK, RF = T.FS, T.BLK, T.RF
N_IQ, SIGMA = T.N_IQ, T.SIGMA
N_EPOCHS = T.N_EPOCHS
MAX_CAND = 30
start_epoch = T.start_epoch
EXTRA_MSEED = 950
EARLY_T0, LATE_T0 = -0.12, 1.20                                         # starts (s from the slot's start) of the early and the late transmission
SHADOWED_AMP, SHADOW_AMP = 6000.0, 0.72                                   # the shadowed transmission's amplitude; the shadow's relative to it


def extra_transmissions(e):
    """[(audio Hz of tone 0, start s -- may be negative, amplitude, message seed)] this module adds to harvest_twin_cases' of slot e."""
    m = EXTRA_MSEED + 10 * e
    return [(1100.0 + 30.0 * e, EARLY_T0, T.STRONG, m), (1700.0 + 30.0 * e, LATE_T0, T.STRONG, m + 1), (2225.0, 0.50, SHADOWED_AMP, m + 2)]


def shadowed_transmission(e):
    return extra_transmissions(e)[2]


def sent_tones(mseed):
    return D.tones_of(C.encode(SEED, C.chain_message(mseed)))


def _iq_of_tones(n, rf_hz, audio_hz, t0_s, amp, tones):
    """ft4_decode_cases.iq_of_tones for a start that may lie before the slot: the samples before sample 0 and after sample n are cut off."""
    ph = S4._phase(np.asarray(tones), rf_hz + audio_hz, T.NSPS, FS)
    sig = amp * np.exp(1j * ph)
    out = np.zeros(n, np.complex64)
    i0 = int(round(t0_s * FS))
    a, b = max(i0, 0), min(i0 + len(sig), n)
    out[a:b] = sig[a - i0:b - i0]
    return out


@functools.lru_cache(maxsize=None)
def slot_iq(e):
    """One slot of IQ (complex64, read-only): harvest_twin_cases' slot e with the extra transmissions and the shadow added."""
    iq = np.array(T.slot_iq(e), np.complex64)
    for audio, t0, amp, mseed in extra_transmissions(e):
        iq = iq + _iq_of_tones(len(iq), RF[0], audio, t0, amp, sent_tones(mseed))
    audio, t0, amp, mseed = shadowed_transmission(e)
    iq = iq + _iq_of_tones(len(iq), RF[0], audio, t0, SHADOW_AMP * amp, (sent_tones(mseed) + 2) & 3)
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def frames(k):
    from oracle import oracle as orc
    oc = orc.Channel(MODE, FS, BLK, RF[k])
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
    """Every stage of channel k in slot e on the CPU, the frame spectrum included."""
    from oracle import oracle as orc
    fr = frames(k)[e]
    code, G = C.make_code(SEED)["code"], OC.generator(SEED)
    cands = orc.ft4_candidates(fr, float(RC.SYNC["f_lo"]), float(RC.SYNC["f_hi"]), RC.SYNCMIN_FT4, max_cand)
    recs = orc.ft4_sync_all(fr, cands)
    cx = orc.ft4_bigspec(fr)
    soft = D.soft_dict(*S4.softbits_of_records(orc, cx, recs))
    msg = D.expected(soft, code, *RC.DECODE4)
    osd = X.expected(soft, msg, G, *RC.OSD4)
    return dict(frame=fr, cx=cx, list=cands, sync=recs, soft=soft, msg=msg, osd=osd)


@functools.lru_cache(maxsize=None)
def expected(e, osd=True, max_cand=MAX_CAND):
    """(decodes, reports) of slot e with channel k under the id k."""
    from oracle import oracle as orc
    cs = [chain(k, e, max_cand) for k in range(len(RF))]
    dec, _ = DR.decodes(MODE, [(k, DR.where_ft4(c["sync"]), c["msg"], c["osd"] if osd else None) for k, c in enumerate(cs)])
    rep = R4.reports(orc, K.encoder(SEED), {k: c["cx"] for k, c in enumerate(cs)}, {k: c["sync"] for k, c in enumerate(cs)}, dec)
    return dec, rep


# ---- the physics of the restatement: on-frequency transmissions in white noise -------------------------------------------------------------------------
PHYS_AMPS = (1200.0, 2400.0, 4800.0, 9600.0)                            # four injected levels 6.02 dB apart, one slot each
PHYS_HZ = (500.0, 1100.0, 1700.0, 2300.0)                               # tone 0 of the four transmissions of a slot
PHYS_T0 = 0.5                                                           # their start, s
PHYS_SIGMA = SIGMA                                                      # per component of the complex noise at FS
PHYS_NOISE_SEED, PHYS_MSEED = 78, 720


def injected_snr_db(amp):
    """SNR in 2500 Hz of a complex carrier of amplitude amp in complex white noise of PHYS_SIGMA per component at FS samples per second."""
    return 10.0 * np.log10(amp ** 2 / (2.0 * PHYS_SIGMA ** 2 * 2500.0 / FS))


@functools.lru_cache(maxsize=None)
def physics():
    """-> [(level index, Hz, injected dB, reported dB, nsymerr)]: the restatement's report at the transmissions' own refined records (the sync
    record of the oracle's search nearest in frequency, strongest sync) with the tones that were sent."""
    from oracle import oracle as orc
    oc = orc.Channel(MODE, FS, BLK, RF[0])
    assert oc.boundary(start_epoch(0)) is None
    out = []
    for lv, amp in enumerate(PHYS_AMPS):
        rng = np.random.default_rng(PHYS_NOISE_SEED + lv)
        iq = (rng.normal(0.0, PHYS_SIGMA, N_IQ) + 1j * rng.normal(0.0, PHYS_SIGMA, N_IQ)).astype(np.complex64)
        for q, hz in enumerate(PHYS_HZ):
            iq = iq + _iq_of_tones(N_IQ, RF[0], hz, PHYS_T0, amp, sent_tones(PHYS_MSEED + q))
        oc.push_many(iq.astype(np.complex64))
        fr = oc.boundary(start_epoch(lv + 1))["i16"]
        cx = orc.ft4_bigspec(fr)
        recs = orc.ft4_sync_all(fr, orc.ft4_candidates(fr, float(RC.SYNC["f_lo"]), float(RC.SYNC["f_hi"]), RC.SYNCMIN_FT4, 100))
        for q, hz in enumerate(PHYS_HZ):
            near = [r for r in recs if abs(r["f1_hz"] - hz) <= 3.0]
            assert near, (lv, hz)
            r = max(near, key=lambda r: r["sync"])
            rep = R4.report(R4.baseband(orc, cx, r["f1_hz"]), r["ibest"], sent_tones(PHYS_MSEED + q))
            out.append((lv, hz, float(injected_snr_db(amp)), float(rep["snr_db"]), int(rep["nsymerr"])))
    oc.close()
    return tuple(out)
