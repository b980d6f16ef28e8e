"""Test helper: FT4 slots in which one message is sent at two or three audio frequencies of one channel, so that one word comes back on several
sync records and cwslg_fetch_decodes has to de-duplicate it and to choose by rank (BP before OSD, then fewer hard errors, then the smaller
entry) -- and what the call must hand out for them, computed on the CPU alone as tests/harvest_cases.py does for FT8: oracle.Channel -> the
restatements of every stage -> tests/decodes_ref.py.

Two channels on one receiver, under record_race_cases' settings but for the list limit: channel 0 (record_race_cases' first FT4 dial offset)
hears the transmissions, channel 1 (the second) hears noise alone -- it has a list and, unless OSD "finds" a word in noise, no decode.
tests/test_harvest_twin_inputs.py proves what the slots contain; amplitudes, frequencies and seeds were searched on the CPU with the
restatements."""
import functools

import numpy as np

import decodes_ref as DR
import ft4_decode_cases as D
import ft4_osd_cases as X
import ft4_softbits_ref as S4
import ldpc_cases as C
import osd_cases as OC
import record_race_cases as RC

MODE = "FT4"
SEED = RC.SEED
FS, BLK, RF = RC.FS, RC.BLK[MODE], RC.RF[MODE]
N_IQ, SIGMA = RC.N_IQ[MODE], RC.SIGMA[MODE]
N_EPOCHS = 2
MAX_CAND = 20
NOISE_SEED = 9400
start_epoch = functools.partial(RC.start_epoch, MODE)
STRONG = 1600.0
NSPS = int(round(FS * 0.048))                                           # samples per symbol
FADE = tuple(range(37, 66)) + tuple(range(70, 99))                      # data symbols between the Costas blocks, in the order a fade takes them

# Slot e, channel 0: [(audio Hz of tone 0, start s, amplitude, message seed[, faded symbols])].  A loud transmission that fades for 28 data
# symbols keeps its place at the head of the list (the list is in the order of the candidate search, strongest first) while belief propagation
# fails on it and OSD recovers it: its copy of ordinary strength comes later in the list and decodes by BP.
TRANSMISSIONS = (
    # 600 twice by BP; 601 and 602 each by OSD on a small entry and by BP on a larger one
    ((300.0, 0.80, STRONG, 600), (800.0, 0.35, 2000.0, 601, 28), (1400.0, 0.30, STRONG, 600), (2000.0, 0.55, 1400.0, 601), (2450.0, 0.45, 2400.0, 602, 28),
     (2750.0, 0.40, 1300.0, 602)),
    # 610 three times by BP; 611 twice, faded both times
    ((300.0, 0.80, STRONG, 610), (800.0, 0.35, 2000.0, 611, 28), (1400.0, 0.30, STRONG, 610), (2450.0, 0.45, 2400.0, 611, 28), (2750.0, 0.40, 1300.0, 610)),
)
assert len(TRANSMISSIONS) == N_EPOCHS


def sent_bits(mseed):
    """bits[12] of a record that carries the message of seed mseed."""
    return np.packbits(np.concatenate([C.chain_message(mseed), np.zeros(5, np.uint8)])).tobytes()


@functools.lru_cache(maxsize=None)
def slot_iq(e):
    """One slot of IQ (complex64, read-only): noise of the slot's own seed and channel 0's transmissions."""
    rng = np.random.default_rng(NOISE_SEED + e)
    iq = (rng.normal(0.0, SIGMA, N_IQ) + 1j * rng.normal(0.0, SIGMA, N_IQ)).astype(np.complex64)
    for audio, t0, amp, mseed, *fade in TRANSMISSIONS[e]:
        tx = D.iq_of_tones(N_IQ, RF[0], audio, t0, amp, D.tones_of(C.encode(SEED, C.chain_message(mseed))))
        for sym in FADE[:fade[0]] if fade else ():                      # a fade: these symbols are not heard at all
            i0 = int(round(t0 * FS)) + sym * NSPS
            tx[i0:i0 + NSPS] = 0
        iq = iq + tx
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def frames(k):
    """The oracle's int16 frame of every slot of channel k, the channel driven as the tests drive the library."""
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
    """Every stage of channel k in slot e, as record_race_cases.chain returns it."""
    from oracle import oracle as orc
    fr = frames(k)[e]
    code, G = C.make_code(SEED)["code"], OC.generator(SEED)
    cands = orc.ft4_candidates(fr, float(RC.SYNC["f_lo"]), float(RC.SYNC["f_hi"]), RC.SYNCMIN_FT4, max_cand)
    recs = orc.ft4_sync_all(fr, cands)
    soft = D.soft_dict(*S4.softbits_of_records(orc, orc.ft4_bigspec(fr), recs))
    msg = D.expected(soft, code, *RC.DECODE4)
    osd = X.expected(soft, msg, G, *RC.OSD4)
    return dict(frame=fr, list=cands, sync=recs, soft=soft, msg=msg, osd=osd)


def channel_input(ch_id, k, e, osd=True):
    """decodes_ref's input for channel index k (library id ch_id) in slot e."""
    c = chain(k, e)
    return ch_id, DR.where_ft4(c["sync"]), c["msg"], c["osd"] if osd else None


def expected(ch_ids, e, osd=True, max_out=None):
    """(records, n_total) cwslg_fetch_decodes must return for slot e: ch_ids[k] is the library's id of channel index k."""
    return DR.decodes(MODE, [channel_input(ch_ids[k], k, e, osd) for k in range(len(ch_ids))], max_out)
