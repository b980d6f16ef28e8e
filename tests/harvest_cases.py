"""Test helper: the slots of tests/test_gpu_fetch_decodes.py and what cwslg_fetch_decodes must hand out for them, computed on the CPU alone --
tests/record_race_cases.py's machinery (oracle.Channel -> the restatements of every stage) followed by tests/decodes_ref.py.

FT8: three slots of this module's own, made so that one transmission comes back on more than one list entry.  Two channels on one receiver:
channel 0 (the first FT8 dial offset of record_race_cases) hears three transmissions of amplitude 2500 per slot, of which the second starts half
a search step (20 ms) and sits half a bin (1.5625 Hz) off the grid and the third starts 0.45 of a step off it; channel 1 (the second dial offset)
hears noise alone: at syncmin 1.2 it has a list and, unless OSD "finds" a word in noise, no decode.  tests/test_harvest_inputs.py proves what
the slots contain.  FT4: the first three slots of record_race_cases itself, under its own settings."""
import functools

import numpy as np

import decodes_ref as DR
import ft8_softbits_ref as S8
import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O
import record_race_cases as RC

SEED = RC.SEED
FS, BLK, RF = RC.FS, RC.BLK, RC.RF
MODES = RC.MODES
N_EPOCHS = 3
FT8_L = (3, 8, 27)                                                      # slot e: the transmissions start L[e] search steps (40 ms) into the slot, plus their own offsets
FT8_MSEED = (810, 800, 820)                                             # slot e: message seeds MSEED[e] .. + 3 (searched on the CPU; test_harvest_inputs.py proves what they give)
NOISE_SEED = 1
AMP, WEAK = 2500.0, 800.0
SYNCMIN8 = 1.2
MAX_CAND = 100
SYNC8 = dict(RC.SYNC, syncmin=SYNCMIN8)
start_epoch, epoch_index = RC.start_epoch, RC.epoch_index


def transmissions8(e):
    """[(audio Hz of tone 0, start s, amplitude, message seed)] of FT8 channel 0 in slot e: three strong ones -- on the grid but for half a step in
    time; half a bin and half a step off it; 0.45 of a step off it -- and a weak one on the grid, in the range belief propagation fails on."""
    L, m = FT8_L[e], FT8_MSEED[e]
    return [(3.125 * 160, 0.04 * (L + 0.5), AMP, m), (3.125 * 480.5, 0.04 * (L + 4.5), AMP, m + 1), (3.125 * 700, 0.04 * (L + 2.45), AMP, m + 2),
            (3.125 * 880, 0.04 * (L + 7), WEAK, m + 3)]


def sent_bits(mseed):
    """bits[12] of a record that carries the message of seed mseed."""
    return np.packbits(np.concatenate([C.chain_message(mseed), np.zeros(5, np.uint8)])).tobytes()


@functools.lru_cache(maxsize=None)
def slot_iq(mode, e):
    """One slot of IQ (complex64, read-only)."""
    if mode == "FT4":
        return RC.slot_iq(mode, e)
    n, sigma = RC.N_IQ[mode], RC.SIGMA[mode]
    rng = np.random.default_rng(NOISE_SEED)
    iq = (rng.normal(0.0, sigma, n) + 1j * rng.normal(0.0, sigma, n)).astype(np.complex64)
    for audio, t0, amp, mseed in transmissions8(e):
        iq = iq + C.iq_of_tones(FS, n, RF[mode][0], audio, t0, amp, C.tones_of(C.encode(SEED, C.chain_message(mseed))))
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq


@functools.lru_cache(maxsize=None)
def frames8(k):
    """The oracle's int16 frame of every FT8 slot of channel k, the channel driven as the tests drive the library."""
    from oracle import oracle as orc
    oc = orc.Channel("FT8", FS, BLK["FT8"], RF["FT8"][k])
    assert oc.boundary(start_epoch("FT8", 0)) is None
    out = []
    for e in range(N_EPOCHS):
        oc.push_many(slot_iq("FT8", e))
        r = oc.boundary(start_epoch("FT8", e + 1))
        assert r is not None and r["t_start"] == start_epoch("FT8", e)
        out.append(r["i16"])
    oc.close()
    return tuple(out)


@functools.lru_cache(maxsize=None)
def chain(mode, k, e, max_cand):
    """Every stage of channel k in slot e with the list limit max_cand, as record_race_cases.chain returns it."""
    if mode == "FT4":
        return RC.chain(mode, k, e, max_cand)
    from oracle import oracle as orc
    fr = frames8(k)[e]
    code, G = C.make_code(SEED)["code"], OC.generator(SEED)
    cands = orc.ft8_sync(fr, SYNC8["f_lo"], SYNC8["f_hi"], SYNC8["syncmin"], max_cand)
    llr, sigma, nsync = S8.softbits(orc.ft8_spectra(fr, S8.soft_pitch(SYNC8["f_hi"])), cands)
    msg = R.hard_records(code, llr, RC.DECODE8[0], nsync, sigma, RC.DECODE8[1])
    osd = O.chain_records(G, llr, RC.OSD8[0], nsync, msg, RC.OSD8[1])
    return dict(frame=fr, list=cands, soft=(llr, sigma, nsync), msg=msg, osd=osd)


def channel_input(mode, ch_id, k, e, max_cand, osd=True):
    """decodes_ref's input for channel index k (library id ch_id) in slot e."""
    c = chain(mode, k, e, max_cand)
    where = DR.where_ft8(c["list"]) if mode == "FT8" else DR.where_ft4(c["sync"])
    return ch_id, where, c["msg"], c["osd"] if osd else None


def expected(mode, ch_ids, e, max_cand, osd=True, max_out=None, only=None):
    """(records, n_total) cwslg_fetch_decodes must return for slot e: ch_ids[k] is the library's id of channel index k; only: the channel indices
    that take part (default: all)."""
    ks = range(len(ch_ids)) if only is None else only
    return DR.decodes(mode, [channel_input(mode, ch_ids[k], k, e, max_cand, osd) for k in ks], max_out)
