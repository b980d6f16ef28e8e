"""Test helper: the large mixed batches of tests/test_gpu_decode_batches.py and the 37-channel FT8 case of tests/test_gpu_decode_many_channels.py,
under the two test codes of tests/ldpc_cases.py, with the restatements' records computed once.  tests/test_decode_batch_inputs.py shows on the CPU,
with the restatements alone, what the batches are FOR (every exit, every branch of the arithmetic, every kind of OSD winner) and that the
many-channel recipe decodes where it says; if a condition fails there, the recipe here changes, not the assertion.

The batch: 1025 sets of 174 metrics per code -- 256 full workgroups of the decode kernels and one wave of the next.  Every set is a codeword
(ldpc_cases.encode of a message91) in noise, llr = scale 2.83 (s + level N(0, 1)), the level drawn per set from [0.3, 1.1] and the scale from
{0.25, 1, 1, 1, 4, 16}.  At positions scattered over the batch by a fixed permutation (so that every family meets ordinary sets in its
workgroups), short families replace the set drawn there:
  rounded  2 (s + 0.9 N(0, 1)) rounded to whole numbers: exact ties in |llr|, exact zeros (the hard decision of +0 is 0), exact distance ties
  zeroed   30 % of the set's metrics are +0
  scaled   the set at scale 1 times 2^-130 (subnormal metrics), 2^-20, 2^40 and 2^120
  inf      one metric of the set is +inf or -inf: defined for belief propagation (T(+-inf) = +-1, no inf - inf arises), not attempted by OSD
  nan      one metric of the set is NaN: not attempted by OSD; the decode's contract expects finite metrics, so these sets are NOT compared
           there (the restatement does not attempt them) -- the GPU tests assert only 0 <= iters <= max_iter on them
  badcrc   a codeword whose CRC field is wrong in little noise: nbad == 0 without crc_ok
OSD runs on a sub-batch of 261 of the 1025 (65 workgroups and one wave) that holds members of every family."""
import functools

import numpy as np

import ldpc_cases as C
import ldpc_ref as R
import osd_cases as OC
import osd_ref as O

F32 = np.float32
N, K = R.N, R.K
SEEDS = C.SEEDS
NSETS = 1025
MAX_ITERS = (5, 30, 200)
ORDERS = (0, 1, 2)
SCALES = (0.25, 1.0, 1.0, 1.0, 4.0, 16.0)
SCALED_EXPONENTS = (-130, -20, 40, 120)
FAMILIES = (("rounded", 40), ("zeroed", 40), ("scaled", 32), ("inf", 24), ("nan", 24), ("badcrc", 6))
OSD_PICK = dict(rounded=30, zeroed=20, scaled=32, inf=12, nan=12, badcrc=6)          # members of each family in the OSD sub-batch
NOSD = 261
# the generator seed of each code's batch: 99 under the first code draws no set that converges after iteration 30 at max_iter 200 (the second code
# has seven there), 105 draws several under either code -- tests/test_decode_batch_inputs.py asserts at least one
BATCH_RNG = {SEEDS[0]: 105, SEEDS[1]: 99}


@functools.lru_cache(maxsize=None)
def family_positions():
    """-> {family: ascending positions in the batch}: consecutive stretches of one fixed permutation of 0..1024."""
    perm = np.random.default_rng(4099).permutation(NSETS)
    out, k = {}, 0
    for name, n in FAMILIES:
        out[name] = np.sort(perm[k:k + n])
        k += n
    return out


@functools.lru_cache(maxsize=None)
def batch(seed):
    """-> dict(llr float32[1025, 174], sent uint8[1025, 91], kind [1025] of str ("cw" or a family's name), nan bool[1025],
    scale float[1025]: the scale drawn for the set, which the "cw" sets keep); read-only."""
    rng = np.random.default_rng(BATCH_RNG[seed])
    sent = np.stack([C.message91(rng) for _ in range(NSETS)])
    level = rng.uniform(0.3, 1.1, NSETS)
    scale = rng.choice(SCALES, NSETS)
    noise = rng.standard_normal((NSETS, N))
    s = np.stack([2.0 * C.encode(seed, m) - 1.0 for m in sent])
    plain = 2.83 * (s + level[:, None] * noise)                        # the sets at scale 1, float64
    llr = (scale[:, None] * plain).astype(F32)
    kind = np.array(["cw"] * NSETS, dtype=object)
    fam = family_positions()
    frng = np.random.default_rng(1999)
    for name, pos in fam.items():
        kind[pos] = name
    for q in fam["rounded"]:
        llr[q] = np.round(2.0 * (s[q] + 0.9 * noise[q])).astype(F32) + F32(0)          # (+ 0: a rounded -0.0 becomes +0)
    for q in fam["zeroed"]:
        llr[q, frng.random(N) < 0.3] = F32(0)
    for j, q in enumerate(fam["scaled"]):
        llr[q] = (plain[q] * 2.0 ** SCALED_EXPONENTS[j % 4]).astype(F32)
    for j, q in enumerate(fam["inf"]):
        llr[q, frng.integers(0, N)] = F32(np.inf) if j % 2 == 0 else F32(-np.inf)
    for q in fam["nan"]:
        llr[q, frng.integers(0, N)] = F32(np.nan)
    for j, q in enumerate(fam["badcrc"]):
        sent[q] = C.message91(frng, flip_crc=True)
        llr[q] = (2.83 * ((2.0 * C.encode(seed, sent[q]) - 1.0) + 0.1 * j * noise[q])).astype(F32)
    out = dict(llr=llr, sent=sent, kind=kind, nan=np.isnan(llr).any(axis=1), scale=scale)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def ldpc_reference(seed, max_iter):
    """The restatement's records of batch(seed); the NaN sets are not attempted (and never compared).  Computed once, shared, read-only."""
    b = batch(seed)
    rec = R.decode(C.make_code(seed)["code"], b["llr"], max_iter, ~b["nan"])
    rec.setflags(write=False)
    return rec


@functools.lru_cache(maxsize=None)
def osd_index():
    """The 261 positions of the OSD sub-batch, ascending: OSD_PICK members of each family (the first of each) and the first ordinary sets."""
    fam = family_positions()
    pick = np.concatenate([fam[name][:n] for name, n in OSD_PICK.items()])
    taken = set(int(q) for pos in fam.values() for q in pos)
    plain = [q for q in range(NSETS) if q not in taken][:NOSD - len(pick)]
    idx = np.sort(np.concatenate([pick, plain]).astype(int))
    assert len(idx) == NOSD == len(set(idx.tolist()))
    idx.setflags(write=False)
    return idx


@functools.lru_cache(maxsize=None)
def osd_sets(seed):
    llr = np.ascontiguousarray(batch(seed)["llr"][osd_index()])
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def osd_reference(seed, order):
    """The restatement's records of osd_sets(seed): computed once, shared, read-only."""
    rec = O.decode(OC.generator(seed), osd_sets(seed), order)
    rec.setflags(write=False)
    return rec


# ---- the contract's decoder against a textbook one: 300 codewords of the first code ------------------------------------------------------------
F64_SEED, F64_LEVELS, F64_PER_LEVEL = SEEDS[0], (0.5, 0.62, 0.7, 0.8, 0.9), 60


@functools.lru_cache(maxsize=None)
def f64_inputs():
    """-> (llr float32[5, 60, 174], sent uint8[5, 60, 91]) from one default_rng(777): per level the 60 messages first, then the noise."""
    rng = np.random.default_rng(777)
    llr, sent = [], []
    for level in F64_LEVELS:
        m = np.stack([C.message91(rng) for _ in range(F64_PER_LEVEL)])
        s = np.stack([2.0 * C.encode(F64_SEED, x) - 1.0 for x in m])
        llr.append((2.83 * (s + level * rng.standard_normal((F64_PER_LEVEL, N)))).astype(F32))
        sent.append(m)
    return np.stack(llr), np.stack(sent)


# ---- 37 FT8 channels on one 48 kHz receiver, one boundary ---------------------------------------------------------------------------------------
# Dials 1150 Hz apart (a 6 kHz channel must end inside the 48 kHz: the highest dial is 17900) with the search range 200..1300 Hz: a transmission
# of channel p at audio a lies in channel p - 1 at a + 1150 and in channel p + 1 at a - 1150, both outside the range for 250 <= a <= 1150, so a probe's message can reach another channel's records only through a
# pointer table in the wrong order or with a wrong stride.  Six probe channels (first, last, the adjacent 17 / 18, 9 and 27) carry two or three
# transmissions of real codewords, (audio Hz of tone 0, start s, amplitude, message seed, stage), every audio frequency, start time and message
# seed unique to its transmission; tones sit on the search grid (3.125 Hz, 40 ms).  Noise as in ldpc_cases.CHAIN.  Amplitudes of the kind
# ldpc_cases.CHAIN uses decode by belief propagation ("bp"); the weakened ones (searched on the CPU oracle's frames as osd_cases.CHAIN's were) fail
# belief propagation at 30 iterations and come out of OSD at order 1 ("osd").  tests/test_decode_batch_inputs.py proves every stage.
MANY_SEED = SEEDS[0]
MANY_FS, MANY_BLK, MANY_N, MANY_SIGMA = C.CHAIN_FS, C.CHAIN_BLK, C.CHAIN_N, C.CHAIN_SIGMA
MANY_DIALS = [-23500 + 1150 * k for k in range(37)]
MANY_SYNC = dict(syncmin=1.2, f_lo=200, f_hi=1300, max_cand=100)
MANY_MAX_ITER, MANY_MIN_NSYNC, MANY_ORDER, MANY_OSD_MIN_NSYNC = 30, 7, 1, 7
MANY_PROBES = {
    0: [(300.0, 0.52, 1100.0, 401, "bp"), (700.0, 1.00, 800.0, 402, "osd"), (1100.0, 0.20, 1300.0, 403, "bp")],
    9: [(350.0, 0.60, 950.0, 404, "bp"), (850.0, 1.40, 1200.0, 405, "bp")],
    17: [(400.0, 0.32, 820.0, 406, "osd"), (1000.0, 0.80, 1000.0, 407, "bp")],
    18: [(462.5, 1.20, 860.0, 408, "osd"), (912.5, 0.40, 1000.0, 409, "bp")],
    27: [(525.0, 0.72, 1200.0, 410, "bp"), (775.0, 1.12, 800.0, 411, "osd"), (1150.0, 0.28, 800.0, 412, "osd")],
    36: [(575.0, 0.92, 900.0, 413, "osd"), (1050.0, 0.44, 1100.0, 414, "bp")],
}
MANY_NOISE_ONLY = (3, 30)
MANY_LAUNCHES = 3          # per boundary with soft bits, decode and OSD on: what the three-channel test_off_means_off (test_gpu_ft8_osd.py) shows


def many_message(mseed):
    return C.message91(np.random.default_rng(mseed))


@functools.lru_cache(maxsize=None)
def many_iq():
    """The slot of IQ (complex64[MANY_N]) under the code of MANY_SEED."""
    rng = np.random.default_rng(4343)
    iq = (rng.normal(0.0, MANY_SIGMA, MANY_N) + 1j * rng.normal(0.0, MANY_SIGMA, MANY_N)).astype(np.complex64)
    for p, txs in MANY_PROBES.items():
        for audio, t0, amp, mseed, stage in txs:
            iq = iq + C.iq_of_tones(MANY_FS, MANY_N, MANY_DIALS[p], audio, t0, amp, C.tones_of(C.encode(MANY_SEED, many_message(mseed))))
    iq = iq.astype(np.complex64)
    iq.setflags(write=False)
    return iq


def many_candidate(cands, tx):
    """Index of the strongest list entry at the transmission's bin and lag (softbits_cases.ft8_best: dt_s = t0 - 0.46 s for a start on the grid)."""
    want = int(round(tx[0] / 3.125))
    near = [q for q, c in enumerate(cands) if c[0] == want and abs(c[4] - (tx[1] - 0.46)) <= 0.03]
    assert near, ("transmission not in the list", tx[:2], [c for c in cands if abs(c[0] - want) <= 2][:5])
    return max(near, key=lambda q: cands[q][2])


def assert_many_channel(p, cands, msg, osd):
    """The conditions of one channel's records, asserted on the CPU for the oracle's frames and on the GPU for the library's records: each of its
    transmissions has crc_ok from the stated stage at its own candidate and carries the message sent; no crc_ok record, from either stage, carries
    another channel's probe message.  -> the stages seen."""
    seen = set()
    for tx in MANY_PROBES.get(p, ()):
        audio, t0, amp, mseed, stage = tx
        q = many_candidate(cands, tx)
        if stage == "bp":
            assert msg[q]["crc_ok"] == 1 and msg[q]["nbad"] == 0 and osd[q].tobytes() == O.NOT_ATTEMPTED.tobytes(), (p, mseed, msg[q], osd[q])
            bits = R.unpack_bits(msg[q]["bits"])
        else:
            assert msg[q]["iters"] >= 1 and msg[q]["crc_ok"] == 0 and osd[q]["crc_ok"] == 1, (p, mseed, msg[q], osd[q])
            bits = R.unpack_bits(osd[q]["bits"])
        assert np.array_equal(bits, many_message(mseed)), (p, mseed)
        seen.add(stage)
    foreign = {R.pack_bits(many_message(tx[3])).tobytes(): (o, tx[3]) for o, txs in MANY_PROBES.items() if o != p for tx in txs}
    for rec in (msg, osd):
        for r in rec[rec["crc_ok"] == 1]:
            assert r["bits"].tobytes() not in foreign, (p, foreign[r["bits"].tobytes()])
    return seen
