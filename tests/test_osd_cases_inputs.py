"""CPU: the inputs of tests/test_gpu_ft8_osd.py, checked with the restatements alone (tests/osd_ref.py, tests/ldpc_ref.py): what each shared metric
set is for, under both test codes, and the chain case on the CPU oracle's frames.  If a property is missing the inputs in tests/osd_cases.py
change, not these assertions."""
import numpy as np
import pytest

import ft8_softbits_ref as S
import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O

I = OC.IDX


@pytest.mark.parametrize("seed", C.SEEDS)
def test_metric_sets_are_what_they_are_for(seed):
    llr, sent = OC.metric_sets(seed)
    assert llr.shape == (12, 174) and llr.dtype == np.float32 and max(OC.BATCHES) <= len(llr)
    r0, r1, r2 = (OC.reference_records(seed, o) for o in OC.ORDERS)
    bp = OC.bp_records(seed)
    bits = lambda r: R.unpack_bits(r["bits"])
    # a clean codeword: the order-0 word at distance +0 at every order
    for r in (r0, r1, r2):
        c = r[I["clean"]]
        assert c["how"] == 0 and c["dmin"] == 0 and c["nharderr"] == 0 and c["crc_ok"] == 1 and np.array_equal(bits(c), sent[I["clean"]])
    # noisy codewords belief propagation (30 iterations) fails on and OSD returns with crc_ok and the sent bits
    for name in ("h1", "h2", "o2"):
        assert bp[I[name]]["iters"] >= 0 and bp[I[name]]["crc_ok"] == 0, name
    h1 = r2[I["h1"]]
    assert h1["how"] == 1 and h1["crc_ok"] == 1 and np.array_equal(bits(h1), sent[I["h1"]]) and h1["nharderr"] > 0
    assert r1[I["h1"]] == h1 and not np.array_equal(bits(r0[I["h1"]]), sent[I["h1"]])                  # order 1 finds it too, order 0 does not
    for name in ("h2", "o2"):
        h2 = r2[I[name]]
        assert h2["how"] == 2 and h2["crc_ok"] == 1 and np.array_equal(bits(h2), sent[I[name]]) and h2["flip"][0] < h2["flip"][1] < 91
        assert not np.array_equal(bits(r1[I[name]]), sent[I[name]])                                     # wrong at order 1, right at order 2
        assert r1[I[name]]["dmin"] > h2["dmin"]
    # a codeword with a wrong CRC
    b = r2[I["badcrc"]]
    assert b["how"] == 0 and b["dmin"] == 0 and b["crc_ok"] == 0 and np.array_equal(bits(b), sent[I["badcrc"]])
    # pure noise: some codeword, far away
    n = r2[I["noise"]]
    assert n["how"] != 0xff and n["nharderr"] > 10 and n["dmin"] > 0
    # signs: all |llr| equal, the order falls back to the index -- the basis is the first 91 independent positions, which for these codes
    # (systematic: message ++ parity) are positions 0..90 themselves: nskip == 0, and the order-0 word repeats the hard decision's first 91 bits
    s = r2[I["signs"]]
    assert len(set(np.abs(llr[I["signs"]]))) == 1 and r0[I["signs"]]["nskip"] == 0
    assert np.array_equal(bits(r0[I["signs"]]), (llr[I["signs"]][:91] > 0).astype(np.uint8))
    assert s["dmin"] == 3 * s["nharderr"]
    # zeros: every distance is +0 and the tie rule picks c0, the all-zero word, at every order
    for r in (r0, r1, r2):
        z = r[I["zeros"]]
        assert z["how"] == 0 and z["dmin"].tobytes() == bytes(4) and not z["bits"].any() and z["nskip"] == 0 and z["nharderr"] == 0 and z["crc_ok"] == 1
    # two equal-distance winners that the flip-count rule separates: all 4187 distances of the order-2 search, the minimum is reached by words
    # of different flip counts, every distance is a whole number, and the record carries the fewest flips among them
    tl = llr[I["tie"]]
    a, hard = np.abs(tl), (tl > 0).astype(np.uint8)
    assert np.array_equal(a, np.round(a))
    pos, nskip, g = O.most_reliable_basis(OC.generator(seed), O.reliability_order(a))
    c0 = ((hard[pos].astype(int) @ g.astype(int)) % 2).astype(np.uint8)
    words, flips = O.candidates(g, c0, 2)
    d = O.distances(words ^ hard[None, :], a)
    tied = sorted(flips[k] for k in np.nonzero(d == d.min())[0])
    assert len({f[0] for f in tied}) >= 2, tied
    t = r2[I["tie"]]
    assert (int(t["how"]), int(t["flip"][0]), int(t["flip"][1])) == tied[0] and t["dmin"] == d.min()
    assert tied[0][0] < tied[-1][0]
    # nskip > 0 and nskip == 0 both occur
    assert r2[I["h2"]]["nskip"] > 0 or r2[I["h1"]]["nskip"] > 0 or r2[I["o2"]]["nskip"] > 0
    assert r2[I["noise"]]["nskip"] >= 0 and r2[I["zeros"]]["nskip"] == 0
    # a NaN, an inf, a -inf: not attempted
    for name in ("nan", "inf", "ninf"):
        assert not np.isfinite(llr[I[name]]).all() and np.isfinite(llr[I[name]]).sum() == 173
        for r in (r0, r1, r2):
            assert r[I[name]].tobytes() == O.NOT_ATTEMPTED.tobytes()
    # the first nine sets (the largest batch of the GPU test) hold every kind of attempted record, the tie included
    assert I["tie"] < 9


def test_the_second_code_decodes_the_same_metrics_differently():
    a, b = C.SEEDS
    llr = OC.metric_sets(a)[0]
    assert O.decode(OC.generator(b), llr, 2).tobytes() != OC.reference_records(a, 2).tobytes()


@pytest.mark.parametrize("seed", C.SEEDS)
def test_chain_case_has_candidates_bp_fails_on_and_osd_recovers(oracle, seed):
    """The chain case on the CPU oracle's frames (exact mode computes the same frames on the GPU) and the numpy soft-bit restatement, with the
    decode at its upstream settings (30 iterations, nsync >= 7): the strongest candidates of CHAIN_RECOVERED's transmissions fail belief
    propagation and come out of OSD (order 2) with crc_ok and the sent message; CHAIN_BP's are decoded by belief propagation and OSD does not
    attempt them; every list also holds candidates below nsync 7, which neither stage attempts."""
    iq = OC.chain_iq(seed)
    code = C.make_code(seed)["code"]
    G = OC.generator(seed)
    for rf, txs in OC.CHAIN:
        oc = oracle.Channel("FT8", OC.CHAIN_FS, OC.CHAIN_BLK, rf)
        oc.boundary(1)
        oc.push_many(iq)
        fr = oc.boundary(16)
        cands = oracle.ft8_sync(fr["i16"], OC.CHAIN_SYNC["f_lo"], OC.CHAIN_SYNC["f_hi"], OC.CHAIN_SYNC["syncmin"], 200)
        llr, sigma, nsync = S.softbits(oracle.ft8_spectra(fr["i16"], S.soft_pitch(OC.CHAIN_SYNC["f_hi"])), cands)
        msg = R.hard_records(code, llr, OC.CHAIN_MAX_ITER, nsync, sigma, OC.CHAIN_MIN_NSYNC)
        osd = O.chain_records(G, llr, OC.CHAIN_ORDER, nsync, msg, OC.CHAIN_OSD_MIN_NSYNC)
        assert (msg["iters"] == -1).any() and ((osd["how"] == 0xff) == ((msg["iters"] < 0) | (msg["crc_ok"] == 1))).all()
        assert (osd["how"] != 0xff).sum() > (osd["crc_ok"] == 1).sum()                                  # OSD also runs on noise and returns words without crc_ok
        for audio, t0, amp, mseed in txs:
            q = [k for k, c in enumerate(cands) if c[0] == int(round(audio / 3.125))][0]
            if mseed in OC.CHAIN_RECOVERED[seed]:
                assert msg[q]["iters"] >= 1 and msg[q]["crc_ok"] == 0
                assert osd[q]["crc_ok"] == 1 and np.array_equal(R.unpack_bits(osd[q]["bits"]), C.chain_message(mseed))
            if mseed in OC.CHAIN_BP:
                assert msg[q]["crc_ok"] == 1 and osd[q].tobytes() == O.NOT_ATTEMPTED.tobytes()
        if rf == OC.CHAIN[0][0] and seed == C.SEEDS[0]:
            assert {int(osd[q]["how"]) for q in range(len(osd)) if osd[q]["crc_ok"]} == {1, 2}          # both kinds of flips come out of the chain
    # the quiet dial offset: an empty list at QUIET_SYNCMIN, where every transmission is still found
    oc = oracle.Channel("FT8", OC.CHAIN_FS, OC.CHAIN_BLK, OC.QUIET_RF)
    oc.boundary(1)
    oc.push_many(iq)
    fr = oc.boundary(16)
    assert len(oracle.ft8_sync(fr["i16"], OC.CHAIN_SYNC["f_lo"], OC.CHAIN_SYNC["f_hi"], OC.QUIET_SYNCMIN, 200)) == 0
    assert len(oracle.ft8_sync(fr["i16"], OC.CHAIN_SYNC["f_lo"], OC.CHAIN_SYNC["f_hi"], OC.CHAIN_SYNC["syncmin"], 200)) > 0
