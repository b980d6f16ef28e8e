"""CPU: the inputs of tests/test_gpu_ft8_decode.py, checked with the restatement alone (tests/ldpc_ref.py): the shared metric sets reach every exit
of the decode under both test codes, and the chain case's transmissions decode, after at least one iteration, from the CPU oracle's frames.  If an
exit is missing the inputs in tests/ldpc_cases.py change, not these assertions."""
import numpy as np
import pytest

import ft8_softbits_ref as S
import ldpc_cases as C
import ldpc_ref as R


@pytest.mark.parametrize("seed", C.SEEDS)
def test_metric_sets_reach_every_exit(seed):
    llr, sent = C.metric_sets(seed)
    assert llr.shape == (9, 174) and llr.dtype == np.float32 and max(C.BATCHES) == len(llr) and np.isfinite(llr).all()
    r5, r30 = C.reference_records(seed, 5), C.reference_records(seed, 30)
    row = lambda r: (int(r["iters"]), int(r["nbad"]), int(r["nharderr"]), int(r["crc_ok"]))
    # iters == 0: the hard decision is a codeword and the CRC matches
    assert row(r30[0]) == row(r5[0]) == (0, 0, 0, 1) and np.array_equal(R.unpack_bits(r30[0]["bits"]), sent[0])
    # a codeword with a wrong CRC
    assert row(r30[1]) == (0, 0, 0, 0) and np.array_equal(R.unpack_bits(r30[1]["bits"]), sent[1])
    # 0 < iters < max_iter with crc_ok and corrected bits
    for q in (2, 3):
        for r, mi in ((r5, 5), (r30, 30)):
            assert 0 < r[q]["iters"] < mi and r[q]["crc_ok"] == 1 and r[q]["nharderr"] > 0 and r[q]["nbad"] == 0
            assert np.array_equal(R.unpack_bits(r[q]["bits"]), sent[q])
    # the early stop of step 5: not a codeword, left between 10 and max_iter with more than 15 unsatisfied checks
    assert 10 <= r30[4]["iters"] < 30 and r30[4]["nbad"] > 15 and r30[4]["crc_ok"] == 0
    # iters == max_iter at 5 and at 30
    assert r5[4]["iters"] == 5 and r5[4]["nbad"] > 0 and r5[5]["iters"] == 5 and r5[7]["iters"] == 5
    assert r30[7]["iters"] == 30 and 0 < r30[7]["nbad"] and r30[7]["crc_ok"] == 0
    # bits are delivered whether or not they form a codeword
    assert r30[7]["bits"].any() and r30[4]["bits"].any()
    # all +0 metrics: the all-zero word is a codeword of any linear code, and its CRC is 0
    assert row(r30[8]) == (0, 0, 0, 1) and not r30[8]["bits"].any()
    # a not-attempted record (the chain's filter)
    na = R.hard_records(C.make_code(seed)["code"], llr[:2], 30, nsync=[6, 21], sigma=[1.0, 1.0], min_nsync=7)
    assert row(na[0]) == (-1, -1, -1, 0) and not na[0]["bits"].any() and na[1] == r30[1]


def test_the_second_code_decodes_the_same_metrics_differently():
    llr = C.metric_sets(C.SEEDS[0])[0]
    a = C.reference_records(C.SEEDS[0], 30)
    b = R.decode(C.make_code(C.SEEDS[1])["code"], llr, 30)
    assert a.tobytes() != b.tobytes()
    assert a[0]["nbad"] == 0 and b[0]["nbad"] > 0                     # a codeword of the first code is none of the second


@pytest.mark.parametrize("seed", C.SEEDS)
def test_chain_case_decodes_after_at_least_one_iteration(oracle, seed):
    """The chain case on the CPU oracle's frames (exact mode computes the same frames on the GPU): per transmission the strongest candidate at its
    bin has crc_ok, the bits sent and iters >= 1; every list also holds candidates that are not attempted (nsync < 7)."""
    iq = C.chain_iq(seed)
    code = C.make_code(seed)["code"]
    for rf, txs in C.CHAIN:
        oc = oracle.Channel("FT8", C.CHAIN_FS, C.CHAIN_BLK, rf)
        oc.boundary(1)
        oc.push_many(iq)
        fr = oc.boundary(16)
        cands = oracle.ft8_sync(fr["i16"], C.CHAIN_SYNC["f_lo"], C.CHAIN_SYNC["f_hi"], C.CHAIN_SYNC["syncmin"], 200)
        llr, sigma, nsync = S.softbits(oracle.ft8_spectra(fr["i16"], S.soft_pitch(C.CHAIN_SYNC["f_hi"])), cands)
        rec = R.hard_records(code, llr, 30, nsync, sigma, 7)
        assert (rec["iters"] == -1).any() and (rec["iters"] > 0).any()
        for audio, t0, amp, mseed in txs:
            q = [k for k, c in enumerate(cands) if c[0] == int(round(audio / 3.125))][0]
            assert q < 5                                               # it survives the cut at max_cand = 5
            assert rec[q]["crc_ok"] == 1 and rec[q]["iters"] >= 1 and rec[q]["nharderr"] > 0
            assert np.array_equal(R.unpack_bits(rec[q]["bits"]), C.chain_message(mseed))
