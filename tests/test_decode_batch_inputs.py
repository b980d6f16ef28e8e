"""CPU: the inputs of tests/test_gpu_decode_batches.py and tests/test_gpu_decode_many_channels.py (tests/decode_batch_cases.py), checked with the
restatements alone (tests/ldpc_ref.py, tests/osd_ref.py): the 1025-set batches reach every exit of the decode at max_iter 5, 30 and 200 and every
branch of its arithmetic, the 261-set OSD sub-batches hold every kind of winner, exact distance ties and not-attempted records, and the
37-channel recipe decodes, on the CPU oracle's frames, at the stage it states.  If a condition fails the recipe changes, not the assertion.

And one measurement that is independent of the restatements: the contract's decoder (Pade tanh, four-piece atanh, early stop, float32) against a
textbook float64 sum-product decoder (tests/bp_f64_ref.py) on 300 codewords in noise."""
import numpy as np
import pytest

import bp_f64_ref as B64
import decode_batch_cases as D
import ft8_softbits_ref as S
import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O

F32 = np.float32
TINY = np.finfo(np.float32).tiny


# ---- a. every exit ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", D.SEEDS)
def test_the_batch_is_what_it_says(seed):
    b = D.batch(seed)
    llr, kind, fam = b["llr"], b["kind"], D.family_positions()
    assert llr.shape == (D.NSETS, 174) and llr.dtype == np.float32 and llr.flags.c_contiguous and D.NSETS == 4 * 256 + 1
    assert sum(n for _, n in D.FAMILIES) == sum(len(p) for p in fam.values()) == (kind != "cw").sum() and kind[D.NSETS - 1] == "cw"
    r = llr[fam["rounded"]]
    assert np.array_equal(r, np.round(r)) and not np.signbit(r[r == 0]).any() and (r == 0).sum() > 100
    assert all(len(np.unique(np.abs(x))) <= 12 for x in r)                                              # many exact ties in |llr|
    z = llr[fam["zeroed"]]
    assert (0.2 * 174 < (z == 0).sum(axis=1)).all() and not np.signbit(z[z == 0]).any()
    sc = np.abs(llr[fam["scaled"]])
    for j, e in enumerate(D.SCALED_EXPONENTS):
        m = np.median(sc[j::4], axis=1)
        assert len(m) == 8 and (m > 2.0 ** (e - 1)).all() and (m < 2.0 ** (e + 3)).all() and np.isfinite(sc[j::4]).all()
    assert ((sc[0::4] > 0) & (sc[0::4] < TINY)).all()                                                    # 2^-130: every metric a subnormal
    for name, test in (("inf", np.isinf), ("nan", np.isnan)):
        assert (test(llr[fam[name]]).sum(axis=1) == 1).all() and (np.isfinite(llr[fam[name]]).sum(axis=1) == 173).all()
    assert {float(x[np.isinf(x)][0]) for x in llr[fam["inf"]]} == {np.inf, -np.inf}
    assert np.array_equal(np.nonzero(b["nan"])[0], fam["nan"]) and np.isfinite(np.delete(llr, np.concatenate([fam["nan"], fam["inf"]]), axis=0)).all()
    # every NaN set shares its workgroup (four consecutive sets) with sets that are compared
    for q in fam["nan"]:
        assert not b["nan"][4 * (q // 4):4 * (q // 4) + 4].all()
    sc = b["scale"][kind == "cw"]
    assert set(sc.tolist()) == {0.25, 1.0, 4.0, 16.0} and (sc == 1.0).sum() > (sc == 4.0).sum() > 50


@pytest.mark.parametrize("seed", D.SEEDS)
@pytest.mark.parametrize("max_iter", D.MAX_ITERS)
def test_every_exit_is_present(seed, max_iter):
    b = D.batch(seed)
    rec = D.ldpc_reference(seed, max_iter)
    assert (rec["iters"][b["nan"]] == -1).all()
    a = rec[~b["nan"]]
    assert (a["iters"] >= 0).all() and (a["iters"] <= max_iter).all()
    assert (a["iters"] == 0).sum() >= 20
    assert ((a["iters"] == max_iter) & (a["nbad"] > 0)).sum() >= 20                                      # left at the limit
    early = (a["iters"] >= 10) & (a["iters"] < max_iter) & (a["nbad"] > 15)                              # nothing else leaves without a codeword below the limit
    assert early.sum() == ((a["iters"] < max_iter) & (a["nbad"] > 0)).sum()
    if max_iter >= 30:
        assert early.sum() >= 20
    if max_iter == 200:
        assert ((a["iters"] > 30) & (a["nbad"] == 0)).sum() >= 1                                         # converges only after iteration 30
    assert ((a["nbad"] == 0) & (a["crc_ok"] == 0)).sum() >= 1
    # what is decoded with crc_ok is what was sent; the inf sets are attempted like any other
    ok = np.nonzero((rec["crc_ok"] == 1))[0]
    assert len(ok) > 300 and all(np.array_equal(R.unpack_bits(rec[q]["bits"]), b["sent"][q]) for q in ok)
    assert (rec["iters"][D.family_positions()["inf"]] >= 0).all()


# ---- b. every branch of the arithmetic ----------------------------------------------------------------------------------------------------------
def _instrumented_decode(code, llr, max_iter, attempt):
    """ldpc_ref.decode's loop again, statement for statement, with counters on the arguments of T and A and on the products (absent edges are not
    counted: nothing reads them).  -> (records, counters); the caller asserts the records ARE ldpc_ref.decode's, so the copy is a faithful one."""
    llr = np.ascontiguousarray(llr, dtype=F32).reshape(-1, R.N)
    Q = len(llr)
    out = np.zeros(Q, R.MSG_DTYPE)
    out["iters"][~attempt] = out["nbad"][~attempt] = out["nharderr"][~attempt] = -1
    live = np.nonzero(attempt)[0]
    v = np.zeros((Q, R.M * 8), F32)
    ncnt, nclast = np.zeros(Q, int), np.zeros(Q, int)
    rb = np.where(code.present, code.rowbit, 0)
    epos = (8 * np.arange(R.M).reshape(-1, 1) + np.arange(R.ROWMAX)).astype(np.int64)
    seen = dict(T_below=0, T_from=0, A=np.zeros(5, int), subnormal_product=0, T_inf=0)
    it = 0
    while live.size:
        L, vv = llr[live], v[live]
        z = ((L + vv[:, code.slot[:, 0]]) + vv[:, code.slot[:, 1]]) + vv[:, code.slot[:, 2]]
        cw = z > 0
        nbad = ((cw[:, rb] & code.present).sum(axis=2) & 1).sum(axis=1)
        done = (nbad == 0) | (it == max_iter)
        if it > 0:
            ncnt[live] = np.where(nbad - nclast[live] < 0, 0, ncnt[live] + 1)
            done |= (ncnt[live] >= 5) & (it >= 10) & (nbad > 15)
        for j in np.nonzero(done)[0]:
            ok = nbad[j] == 0 and R.crc14(cw[j][:77]) == R.crc_field(cw[j][:R.K])
            out[live[j]] = (R.pack_bits(cw[j]), it, nbad[j], int(((L[j] > 0) != cw[j]).sum()), int(ok), 0)
        nclast[live] = nbad
        live, z, vv = live[~done], z[~done], vv[~done]
        if not live.size:
            break
        x = F32(-0.5) * (z[:, rb] - vv[:, epos])
        ax = np.abs(x[:, code.present])
        seen["T_below"] += int((ax < F32(4.97)).sum())
        seen["T_from"] += int((ax >= F32(4.97)).sum())
        seen["T_inf"] += int(np.isinf(ax).sum())
        t = R.T(x)
        new = vv.copy()
        for e in range(R.ROWMAX):
            p = np.ones((live.size, R.M), F32)
            for f in range(R.ROWMAX):
                if f != e:
                    p = np.where(code.present[:, f], p * t[:, :, f], p)
                    seen["subnormal_product"] += int(((p != 0) & (np.abs(p) < TINY))[:, code.present[:, e]].sum())
            rows = code.present[:, e]
            ap = np.abs(p[:, rows])
            seen["A"] += np.bincount(np.searchsorted(np.array([0.664, 0.9217, 0.9951, 0.9998], F32), ap.ravel(), side="left"), minlength=5)
            new[:, epos[rows, e]] = (F32(2) * R.A(-p))[:, rows]
        v[live] = new
        it += 1
    return out, seen


@pytest.mark.parametrize("seed", D.SEEDS)
def test_every_branch_of_the_arithmetic_is_present(seed):
    b = D.batch(seed)
    rec, seen = _instrumented_decode(C.make_code(seed)["code"], b["llr"], 30, ~b["nan"])
    assert rec.tobytes() == D.ldpc_reference(seed, 30).tobytes()                                          # the instrumented copy is the restatement
    assert seen["T_below"] > 1000 and seen["T_from"] > 1000 and seen["T_inf"] > 0
    assert (seen["A"] > 100).all(), seen["A"]                                                            # z <= 0.664, <= 0.9217, <= 0.9951, <= 0.9998, beyond
    assert seen["subnormal_product"] > 0
    # (searchsorted's "left" puts z == breakpoint into the piece A's "<=" puts it in)
    edges = np.array([0.664, 0.9217, 0.9951, 0.9998], F32)
    assert list(np.searchsorted(edges, edges, side="left")) == [0, 1, 2, 3] and np.searchsorted(edges, np.nextafter(edges[3], F32(2))) == 4


# ---- c. the OSD sub-batch -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", D.SEEDS)
def test_osd_sub_batch_holds_every_kind_of_record(seed):
    idx, llr = D.osd_index(), D.osd_sets(seed)
    b = D.batch(seed)
    assert llr.shape == (261, 174) and len(idx) == 4 * 65 + 1 and np.array_equal(llr.view(np.uint32), b["llr"][idx].view(np.uint32))
    for name, n in D.OSD_PICK.items():
        assert (b["kind"][idx] == name).sum() == n >= 6
    r0, r1, r2 = (D.osd_reference(seed, o) for o in D.ORDERS)
    finite = np.isfinite(llr).all(axis=1)
    for r, order in ((r0, 0), (r1, 1), (r2, 2)):
        assert ((r["how"] == 0xff) == ~finite).all() and (r[finite]["how"] <= order).all()
        assert all(x.tobytes() == O.NOT_ATTEMPTED.tobytes() for x in r[~finite])
    assert (~finite).sum() >= 10
    assert all((r2["how"] == h).sum() >= 5 for h in (0, 1, 2)) and all((r1["how"] == h).sum() >= 5 for h in (0, 1))
    assert (r2["nskip"] > 0).sum() >= 5 and (r2[finite]["nskip"] == 0).sum() >= 1
    # the scaled sets: finite distances from about 1e-38 to about 1e37
    sc = r2[b["kind"][idx] == "scaled"]
    assert np.isfinite(sc["dmin"]).all() and (sc["how"] != 0xff).all() and 0 < sc["dmin"][sc["dmin"] > 0].min() < 1e-36 and sc["dmin"].max() > 1e35
    # exact float32 ties for the minimum that the index rule decides: all 4187 distances again, as tests/test_osd_cases_inputs.py does for its one
    ties, hows = 0, set()
    G = OC.generator(seed)
    for q in np.nonzero(np.isin(b["kind"][idx], ("rounded", "zeroed")))[0]:
        a, hard = np.abs(llr[q]), (llr[q] > 0).astype(np.uint8)
        pos, nskip, g = O.most_reliable_basis(G, O.reliability_order(a))
        c0 = ((hard[pos].astype(int) @ g.astype(int)) % 2).astype(np.uint8)
        words, flips = O.candidates(g, c0, 2)
        d = O.distances(words ^ hard[None, :], a)
        tied = np.nonzero(d == d.min())[0]
        t = r2[q]
        assert (int(t["how"]), int(t["flip"][0]), int(t["flip"][1])) == flips[tied[0]] and t["dmin"] == d.min()
        if len(tied) > 1:
            ties += 1
            hows |= {flips[k][0] for k in tied}
    print("sets with a tie for the minimum", ties, "flip counts among the tied", sorted(hows))
    assert ties >= 5, ties
    # what OSD returns with crc_ok from an ordinary set is, with few exceptions, what was sent (a wrong word with a matching CRC is 1 in 16384)
    ok = np.nonzero((r2["crc_ok"] == 1) & (b["kind"][idx] == "cw"))[0]
    assert len(ok) > 50 and sum(np.array_equal(R.unpack_bits(r2[q]["bits"]), b["sent"][idx[q]]) for q in ok) >= len(ok) - 1


# ---- d. the contract's decoder against a textbook one -------------------------------------------------------------------------------------------
def test_the_contract_decoder_loses_little_against_float64_sum_product():
    """300 codewords of code 1741, 60 at each noise level, through ldpc_ref.decode (30 iterations) and through bp_f64_ref.decode (30 iterations, no
    early stop).  "Correct": returned as a codeword whose CRC matches and equal to the message sent.  Measured with this implementation:

        noise level                 0.5   0.62   0.7   0.8   0.9   total
        restatement correct          60     60    59    41    15     235
        float64 decoder correct      60     60    59    43    14     236

    The conditions are caps, not these measurements: per level the restatement decodes at most 3 sets fewer than the float64 decoder, over all 300
    at most 5 fewer, and no decoder returns a codeword with a matching CRC that is not the message sent."""
    code = C.make_code(D.F64_SEED)["code"]
    llr, sent = D.f64_inputs()
    assert llr.shape == (5, 60, 174) and sent.shape == (5, 60, 91)
    rest, f64 = [], []
    for lv in range(len(D.F64_LEVELS)):
        rec = R.decode(code, llr[lv], 30)
        cw, ok, iters = B64.decode(code, llr[lv], 30)
        assert (iters[~ok] == 30).all() and not ((code.H.astype(int) @ cw[ok].T) % 2).any()
        crc = np.array([R.crc14(w[:77]) == R.crc_field(w[:R.K]) for w in cw])
        good_r = np.array([np.array_equal(R.unpack_bits(r["bits"]), m) for r, m in zip(rec, sent[lv])])
        good_f = (cw[:, :R.K] == sent[lv]).all(axis=1)
        assert good_r[rec["crc_ok"] == 1].all() and good_f[ok & crc].all()                               # nothing wrong is passed off as decoded
        rest.append(int((good_r & (rec["crc_ok"] == 1)).sum()))
        f64.append(int((good_f & ok & crc).sum()))
    print("restatement", rest, sum(rest), "float64", f64, sum(f64))
    assert all(f - r <= 3 for r, f in zip(rest, f64)), (rest, f64)
    assert sum(f64) - sum(rest) <= 5, (rest, f64)
    assert f64[0] == 60 and f64[-1] < 40                                                                 # the levels span "always" to "seldom"


# ---- the 37-channel recipe on the CPU oracle's frames -------------------------------------------------------------------------------------------
def test_many_channel_recipe_decodes_at_the_stated_stages(oracle):
    """The six probe channels and the two noise-only ones of decode_batch_cases.MANY_* through the oracle's chain (exact mode computes the same
    frames on the GPU), the numpy soft-bit restatement, ldpc_ref at 30 iterations and osd_ref at order 1: per probe transmission the strongest
    candidate has crc_ok from the stated stage and carries the message sent; both stages occur; no channel holds another probe's message."""
    assert len(D.MANY_DIALS) == 37 and sorted(D.MANY_PROBES) == [0, 9, 17, 18, 27, 36] and not set(D.MANY_NOISE_ONLY) & set(D.MANY_PROBES)
    txs = [tx for t in D.MANY_PROBES.values() for tx in t]
    for k in (0, 1, 3):                                                                                   # audio, start, message seed: unique
        assert len({tx[k] for tx in txs}) == len(txs) == 14
    assert all(2 <= len(t) <= 3 for t in D.MANY_PROBES.values())
    assert all(250 <= tx[0] <= 1150 and tx[0] % 3.125 == 0 and abs(tx[1] / 0.04 - round(tx[1] / 0.04)) < 1e-9 for tx in txs)
    assert all(abs(f) <= 24000 and f + 6000 <= 24000 for f in D.MANY_DIALS)
    iq = D.many_iq()
    code, G = C.make_code(D.MANY_SEED)["code"], OC.generator(D.MANY_SEED)
    stages = {}
    for p in list(D.MANY_PROBES) + list(D.MANY_NOISE_ONLY):
        oc = oracle.Channel("FT8", D.MANY_FS, D.MANY_BLK, D.MANY_DIALS[p])
        oc.boundary(1)
        oc.push_many(iq)
        fr = oc.boundary(16)
        oc.close()
        cands = oracle.ft8_sync(fr["i16"], D.MANY_SYNC["f_lo"], D.MANY_SYNC["f_hi"], D.MANY_SYNC["syncmin"], D.MANY_SYNC["max_cand"])
        llr, sigma, nsync = S.softbits(oracle.ft8_spectra(fr["i16"], S.soft_pitch(D.MANY_SYNC["f_hi"])), cands)
        msg = R.hard_records(code, llr, D.MANY_MAX_ITER, nsync, sigma, D.MANY_MIN_NSYNC)
        osd = O.chain_records(G, llr, D.MANY_ORDER, nsync, msg, D.MANY_OSD_MIN_NSYNC)
        assert 50 < len(cands) <= D.MANY_SYNC["max_cand"]
        assert (msg["iters"] == -1).any() and (osd["how"] != 0xff).sum() >= 10                            # both gates bite, and there is work to compare
        for tx in D.MANY_PROBES.get(p, ()):
            stages[tx[3]] = tx[4]
        assert D.assert_many_channel(p, cands, msg, osd) == {tx[4] for tx in D.MANY_PROBES.get(p, ())}
        if p in D.MANY_NOISE_ONLY:
            assert not msg["crc_ok"].any() and not osd["crc_ok"].any()
    assert sorted(stages.values()).count("bp") >= 1 and sorted(stages.values()).count("osd") >= 1
