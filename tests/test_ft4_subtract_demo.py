"""CPU: why the FT4 subtractor exists.  A weak transmission sits under a strong one a fraction of a tone spacing to two tone spacings away.  The
CPU chain of restatements -- the oracle's FT4 search and refinement (ft4_candidates, ft4_sync_all, ft4_bigspec), tests/ft4_softbits_ref.py,
tests/ldpc_ref.py through ft4_decode_cases.expected, belief propagation alone -- decodes the strong word from the frame and not the weak one; run
once more on the residual of tests/ft4_subtract_ref.py (the strong word taken out at the record's own f1_hz / dt_s), it decodes the weak one.  The
thirteen recipes are the FT8 demonstration's mapped to FT4: separations scaled by the tone-spacing ratio 10/3 (5 to 41.7 Hz), the same amplitude
ratios (14 to 28 dB), starts on and off the 666.67 Hz sample grid around 0.5 s, one early, one late."""
import functools

import numpy as np
import pytest

import decodes_ref as DR
import ft4_decode_cases as D
import ft4_decode_reports_ref as R4
import ft4_gfsk as G
import ft4_softbits_ref as S4
import ft4_subtract_ref as S
import ldpc_cases as C
import report_kernel_cases as K

SEED = C.SEEDS[0]
SYNC = dict(f_lo=200.0, f_hi=3000.0, syncmin=1.1, max_cand=50)
DECODE = (30, 0, 0)                                                       # max_iter, min_nsync, min_nqual: every record is attempted
F_STRONG = 1203.7
R = 10.0 / 3.0                                                            # FT4's tone spacing over FT8's
# (separation Hz, strong amplitude, weak amplitude, noise sigma per sample, strong start s - 0.5, weak start s - 0.5).  0.001 s is baseband sample
# 334 (on the 666.67 Hz grid), 0.0 s is a third of a sample off it, 0.0115 and -0.0085 lie between grid points; -0.31 is early, 0.55 late
RECIPES = [(3.0 * R, 3000, 300, 1000, 0.001, 0.251), (4.7 * R, 3000, 400, 1000, 0.001, 0.251), (2.0 * R, 5000, 300, 800, 0.001, 0.251),
           (6.25 * R, 3000, 250, 1000, 0.001, 0.251), (9.0 * R, 4000, 300, 1000, 0.001, 0.251), (1.5 * R, 2000, 300, 1000, 0.001, 0.251),
           (3.0 * R, 6000, 250, 800, 0.001, 0.251), (12.5 * R, 3000, 300, 1000, 0.001, 0.251),
           (3.0 * R, 3000, 300, 1000, 0.0, 0.2), (3.0 * R, 3000, 300, 1000, 0.0115, 0.2115), (3.0 * R, 3000, 300, 1000, -0.0085, 0.1915),
           (3.0 * R, 3000, 300, 1000, 0.55, 0.35), (3.0 * R, 3000, 300, 1000, -0.31, -0.06)]


def chain(frame_f32):
    """{bits[12] as bytes: (f1_hz, dt_s) of the first decode that carries the word} -- search, refinement, soft bits, BP on an int16 copy of the
    frame; the decodes are what cwslg_fetch_decodes would emit for the channel (tests/decodes_ref.py), so f1_hz / dt_s are the record's own"""
    from oracle import oracle as orc
    fr = np.clip(np.rint(frame_f32), -32767, 32767).astype(np.int16)
    cands = orc.ft4_candidates(fr, SYNC["f_lo"], SYNC["f_hi"], SYNC["syncmin"], SYNC["max_cand"])
    recs = orc.ft4_sync_all(fr, cands)
    if not recs:
        return {}
    soft = D.soft_dict(*S4.softbits_of_records(orc, orc.ft4_bigspec(fr), recs))
    msg = D.expected(soft, C.make_code(SEED)["code"], *DECODE)
    dec, _ = DR.decodes("FT4", [(0, DR.where_ft4(recs), msg, None)])
    return {bytes(d["bits"]): (d["freq_hz"], d["dt_s"]) for d in dec}


def _pack(m91):
    return bytes(np.packbits(np.concatenate([m91, np.zeros(5, np.uint8)])))


@functools.lru_cache(maxsize=None)
def run(i):
    sep, a_s, a_w, sigma, dt_s, dt_w = RECIPES[i]
    ms, mw = C.chain_message(5000 + 2 * i), C.chain_message(5001 + 2 * i)
    ts, tw = D.tones_of(C.encode(SEED, ms)), D.tones_of(C.encode(SEED, mw))
    strong = G.synth(ts, F_STRONG, dt_s, a_s, 0.3 + i)
    x = strong + G.synth(tw, F_STRONG + sep, dt_w, a_w, 1.1 + i)
    x = (x + sigma * np.random.default_rng(600 + i).standard_normal(S.N)).astype(np.float32)
    frame = chain(x)
    items = [(R4.tones(K.encoder(SEED), np.frombuffer(b, np.uint8)), np.float32(f), np.float32(dt)) for b, (f, dt) in frame.items()]
    recs, res, _ = S.subtract(x, items)
    # the weak transmission alone in the same noise: the recipe is no trick of the noise
    alone = chain((x - strong).astype(np.float32))
    return dict(strong=_pack(ms), weak=_pack(mw), frame=frame, residual=chain(res), alone=alone, recs=recs, order=list(frame))


@pytest.mark.parametrize("i", range(len(RECIPES)))
def test_weak_under_strong_decodes_from_the_residual_only(i):
    """Measured: all thirteen recipes meet the preconditions at the FT8 levels and all thirteen gain the decode.  The refined start lies within
    two time steps of the truth in all thirteen (0 to 1 sample off); the refined frequency within 0.004 Hz of it (a grid step is 0.0781 Hz).
    The two grid searches ALONE miss the frequency bound in recipe 3 (weak transmission exactly one tone spacing above, 21.6 dB down, 5.2 symbols
    later): 0.0916 Hz, because the symbol metric is not coherent across symbols and the neighbour's leak moves its flat maximum by a step; the
    track's phase slope (step 4a of the statement) is coherent over the whole signal and brings it to 0.0014 Hz.  DESIGN.md 4.16 has the figures."""
    r = run(i)
    assert r["weak"] in r["alone"]                                      # decodable on its own
    assert r["strong"] in r["frame"] and r["weak"] not in r["frame"]    # from the frame: the strong word alone
    assert r["weak"] in r["residual"]                                   # from the residual: the weak word
    assert r["strong"] not in r["residual"]                             # and the strong one is gone
    # the refined values are the strong transmission's own: within one frequency-grid step and two time-grid steps of the truth (the record's sit
    # on the 1 Hz grid of the refinement and the 666.67 Hz grid of the baseband)
    sep, a_s, a_w, sigma, dt_s, dt_w = RECIPES[i]
    rec = r["recs"][r["order"].index(r["strong"])]
    print("strong: record f1 %.3f dt %.5f -> fit f %.3f dt %.5f (truth %.1f, %.4f)" % (*r["frame"][r["strong"]], rec["f_hz"], rec["dt_s"], F_STRONG, dt_s))
    assert abs(float(rec["f_hz"]) - F_STRONG) <= S.FREQ_STEP_HZ and abs(float(rec["dt_s"]) - dt_s) <= 2 * S.TIME_STEP_S, rec


def test_recipes_that_gain_a_decode():
    gained = sum(1 for i in range(len(RECIPES)) if run(i)["weak"] in run(i)["residual"] and run(i)["weak"] not in run(i)["frame"])
    print("%d of %d recipes gain a decode" % (gained, len(RECIPES)))
    assert gained == len(RECIPES)
