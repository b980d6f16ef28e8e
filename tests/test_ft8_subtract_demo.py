"""CPU: why the subtractor exists.  A weak transmission sits under a strong one a few hertz away.  The CPU chain of restatements -- the oracle's FT8
search (sync_oracle), tests/ft8_softbits_ref.py, tests/ldpc_ref.py, belief propagation alone -- decodes the strong word from the frame and not the
weak one; run once more on the residual of tests/ft8_subtract_ref.py (the strong word taken out at the candidate's own freq_hz / dt_s), it decodes
the weak one.  Thirteen recipes (separation 1.5 to 12.5 Hz, the strong one 14 to 28 dB above the weak one, five start times on and off the 40 ms
grid): all thirteen gain the decode."""
import functools

import numpy as np
import pytest

import decode_reports_ref as RR
import ft8_gfsk as G
import ft8_softbits_ref as S8
import ft8_subtract_ref as S
import ldpc_cases as C
import ldpc_ref as R
import report_kernel_cases as K

SEED = C.SEEDS[0]
SYNC = dict(f_lo=200, f_hi=3000, syncmin=1.5, max_cand=50)
DECODE = (30, 7)                                                         # max_iter, min_nsync
F_STRONG = 1203.7
# (separation Hz, strong amplitude, weak amplitude, noise sigma per sample, strong start s, weak start s)
RECIPES = [(3.0, 3000, 300, 1000, 0.3, 0.9), (4.7, 3000, 400, 1000, 0.3, 0.9), (2.0, 5000, 300, 800, 0.3, 0.9), (6.25, 3000, 250, 1000, 0.3, 0.9),
           (9.0, 4000, 300, 1000, 0.3, 0.9), (1.5, 2000, 300, 1000, 0.3, 0.9), (3.0, 6000, 250, 800, 0.3, 0.9), (12.5, 3000, 300, 1000, 0.3, 0.9),
           (3.0, 3000, 300, 1000, 0.31, 0.81), (3.0, 3000, 300, 1000, 0.29, 0.79), (3.0, 3000, 300, 1000, 0.27, 0.77), (3.0, 3000, 300, 1000, 1.013, 1.513),
           (3.0, 3000, 300, 1000, -0.31, 0.19)]


def chain(frame_f32):
    """{bits[12] as bytes: (freq_hz, dt_s) of the first list entry that carries the word} -- search, soft bits, BP on an int16 copy of the frame"""
    from oracle import oracle as orc
    fr = np.zeros(240000, np.int16)
    fr[:S.N] = np.clip(np.rint(frame_f32), -32767, 32767).astype(np.int16)
    cands = orc.ft8_sync(fr, SYNC["f_lo"], SYNC["f_hi"], SYNC["syncmin"], SYNC["max_cand"])
    if not cands:
        return {}
    plane = np.ascontiguousarray(orc.ft8_spectra(fr, S8.soft_pitch(SYNC["f_hi"])), np.float32)
    llr, sigma, nsync = S8.softbits(plane, cands)
    msg = R.hard_records(C.make_code(SEED)["code"], llr, DECODE[0], nsync, sigma, DECODE[1])
    out = {}
    for q in range(len(cands)):
        if msg["crc_ok"][q]:
            out.setdefault(bytes(msg["bits"][q]), (cands[q][3], cands[q][4]))
    return out


def _pack(m91):
    return bytes(np.packbits(np.concatenate([m91, np.zeros(5, np.uint8)])))


@functools.lru_cache(maxsize=None)
def run(i):
    sep, a_s, a_w, sigma, dt_s, dt_w = RECIPES[i]
    ms, mw = C.chain_message(5000 + 2 * i), C.chain_message(5001 + 2 * i)
    ts, tw = C.tones_of(C.encode(SEED, ms)), C.tones_of(C.encode(SEED, mw))
    x = G.synth(ts, F_STRONG, dt_s, a_s, 0.3 + i) + G.synth(tw, F_STRONG + sep, dt_w, a_w, 1.1 + i)
    x = (x + sigma * np.random.default_rng(600 + i).standard_normal(S.N)).astype(np.float32)
    frame = chain(x)
    items = [(RR.tones(K.encoder(SEED), np.frombuffer(b, np.uint8)), np.float32(f), np.float32(dt)) for b, (f, dt) in frame.items()]
    recs, res, _ = S.subtract(x, items)
    # the weak transmission alone in the same noise: the recipe is no trick of the noise
    alone = chain((x - G.synth(ts, F_STRONG, dt_s, a_s, 0.3 + i)).astype(np.float32))
    return dict(strong=_pack(ms), weak=_pack(mw), frame=frame, residual=chain(res), alone=alone, recs=recs)


@pytest.mark.parametrize("i", range(len(RECIPES)))
def test_weak_under_strong_decodes_from_the_residual_only(i):
    r = run(i)
    assert r["weak"] in r["alone"]                                      # decodable on its own
    assert r["strong"] in r["frame"] and r["weak"] not in r["frame"]    # from the frame: the strong word alone
    assert r["weak"] in r["residual"]                                   # from the residual: the weak word
    assert r["strong"] not in r["residual"]                             # and the strong one is gone
    # the refined values are the strong transmission's own (the candidate's sit on the 3.125 Hz / 40 ms grid, dt_s one step late)
    sep, a_s, a_w, sigma, dt_s, dt_w = RECIPES[i]
    assert abs(float(r["recs"]["f_hz"][0]) - F_STRONG) <= 0.1 and abs(float(r["recs"]["dt_s"][0]) - dt_s) <= 2 * S.TIME_STEP_S, r["recs"]


def test_recipes_that_gain_a_decode():
    gained = sum(1 for i in range(len(RECIPES)) if run(i)["weak"] in run(i)["residual"] and run(i)["weak"] not in run(i)["frame"])
    print("%d of %d recipes gain a decode" % (gained, len(RECIPES)))
    assert gained == len(RECIPES)
