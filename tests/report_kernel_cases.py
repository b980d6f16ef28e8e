"""Test helper: decode_report_kernel (csrc/harvest_kernels.hpp) on planes, lists and records the test writes -- the cases
of tests/test_gpu_report_kernel.py, the file formats of tests/report_kernel_check.hip, and what the kernel must leave in its report block,
computed by tests/decode_reports_ref.py alone.  tests/test_report_kernel_inputs.py proves what the cases contain.

Also the hand-made planes of tests/test_decode_reports_ref.py and a table whose last 83 columns are singular."""
import functools
import os
import struct
import subprocess

import numpy as np

import decode_reports_ref as RR
import decodes_ref as DR
import ldpc_cases as LC

F32 = np.float32
AB = 0xABABABAB
GUARD_RECS, HEAD_WORDS, REC_WORDS, REP_WORDS = 8, 4, 10, 4              # as in report_kernel_check.hip
CAND = np.dtype([("freq_bin", np.int32), ("time_step", np.int32), ("sync", F32), ("freq_hz", F32), ("dt_s", F32)])
SEED = LC.SEEDS[0]
ALL_ONES = bytes([0xFF] * 11 + [0xE0])                                  # the 91-bit all-ones word


# ---- tables and encoders ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def encoder(seed):
    G = RR.encoder(LC.make_code(seed)["nm"])
    assert G is not None
    G.setflags(write=False)
    return G


def enc_words(G):
    """The encoder in the OsdGen layout: uint32[91][6], codeword bit t at row[t >> 5] bit t & 31."""
    w = np.zeros((RR.K, 6), np.uint32)
    for k in range(RR.K):
        for t in np.nonzero(G[k])[0]:
            w[k, t >> 5] |= np.uint32(1) << np.uint32(t & 31)
    return w


def nm_of(H):
    """A table nm[83][7] with the rows' positions ascending."""
    nm = np.zeros((RR.M, 7), np.uint8)
    for m in range(RR.M):
        cols = np.nonzero(H[m])[0] + 1
        nm[m, :len(cols)] = cols
    return nm


@functools.lru_cache(maxsize=None)
def singular_table(seed):
    """The code of make_code(seed) with one message column and one parity column exchanged so that columns 91..173 become singular: every rule
    of cwslg_set_ldpc_code still holds (weights, rank 83 of the whole H), only the systematic form is gone."""
    H = RR.parity_matrix(LC.make_code(seed)["nm"])
    for a in range(RR.K):
        for b in range(RR.K, RR.N):
            perm = np.arange(RR.N)
            perm[[a, b]] = perm[[b, a]]
            H2 = H[:, perm]
            if LC._gf2_rank_pivots(H2[:, RR.K:])[0] < RR.M:
                assert LC._gf2_rank_pivots(H2)[0] == RR.M
                return nm_of(H2)
    raise AssertionError("no exchange makes the parity columns singular")


def word_of_bits(bits91):
    return np.packbits(np.concatenate([np.asarray(bits91, np.uint8), np.zeros(5, np.uint8)])).tobytes()


# ---- hand-made planes ---------------------------------------------------------------------------------------------------------------------------------
def plane_of_terms(i, j, tones, sig=None, noi=None, pitch=32, fill=0.0):
    """A plane [372, pitch] of `fill` in which symbol n carries sig[n] at its tone and noi[n] at tone (t + 4) mod 7, seen from (i, j); symbols
    outside the plane are skipped."""
    pl = np.full((RR.NHSYM, pitch), fill, F32)
    for n in range(RR.NSYM):
        m = j + 12 + 4 * n
        if not 1 <= m <= RR.NHSYM:
            continue
        t = int(tones[n])
        if noi is not None and i + 2 * ((t + 4) % 7) < pitch:
            pl[m - 1, i + 2 * ((t + 4) % 7)] = noi[n]
        if sig is not None and i + 2 * t < pitch:
            pl[m - 1, i + 2 * t] = sig[n]
    return pl


# ---- kernel cases --------------------------------------------------------------------------------------------------------------------------------------
def _decode(ch_id, entry, word):
    r = np.zeros((), DR.DECODE_DTYPE)
    r["ch_id"], r["entry"], r["bits"] = ch_id, entry, np.frombuffer(word, np.uint8)
    r["ndup"] = 1
    return r


def _cands(ij):
    c = np.zeros(len(ij), CAND)
    for q, (i, j) in enumerate(ij):
        c[q] = (i, j, 2.0 + q, 3.125 * i, 0.04 * j)
    return c


def _noise_plane(rng, pitch, scale=1.0):
    return (rng.random((RR.NHSYM, pitch), F32) * F32(scale)).astype(F32)


def _random_word(rng):
    return word_of_bits(rng.integers(0, 2, RR.K))


def _case(name, channels, per_channel_records, seed=SEED, lim=None, n_total=None):
    """channels: [dict(plane, list)]; per_channel_records: [[(entry, word)]] -- the records of channel c in order.  lim None: everything."""
    recs, offsets = [], []
    for c, rs in enumerate(per_channel_records):
        offsets.append(len(recs))
        recs += [_decode(100 + c, e, w) for e, w in rs]
    recs = np.array(recs, DR.DECODE_DTYPE) if recs else np.zeros(0, DR.DECODE_DTYPE)
    total = len(recs) if n_total is None else n_total
    return dict(name=name, seed=seed, channels=channels, offsets=np.array(offsets, np.uint32), records=recs, n_total=total,
                lim=len(recs) if lim is None else lim)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20260)
    G = encoder(SEED)
    out = []
    # (a) 1, 3, 4, 5, 63, 64, 65 decodes of one channel: a wave within its workgroup, the last partial workgroup
    for nd in (1, 3, 4, 5, 63, 64, 65):
        ij = [(int(rng.integers(0, 18)), int(rng.integers(-62, 63))) for _ in range(16)]
        ch = dict(plane=_noise_plane(rng, 32), list=_cands(ij))
        out.append(_case(f"decodes_{nd}", [ch], [[(int(rng.integers(0, 16)), _random_word(rng)) for _ in range(nd)]]))
    # (b) the plane's edges: j = -62 and +62, i = 0 and the last bin for which tone 7 is inside the pitch, pitches 32 and 992
    for pitch in (32, 992):
        ij = [(0, -62), (0, 62), (pitch - 15, -62), (pitch - 15, 62), (pitch - 15, 0), (0, 0), (pitch - 14, 0), (pitch - 1, 5)]
        ch = dict(plane=_noise_plane(rng, pitch), list=_cands(ij))
        out.append(_case(f"edges_pitch_{pitch}", [ch], [[(e, _random_word(rng)) for e in range(len(ij))]]))
    # (c) a plane of equal values: every first maximum at tone 0
    ch = dict(plane=np.full((RR.NHSYM, 32), 0.25, F32), list=_cands([(3, 1), (0, -62)]))
    out.append(_case("equal_plane", [ch], [[(0, _random_word(rng)), (1, ALL_ONES), (1, _random_word(rng))]]))
    # (d) one huge and 78 tiny terms: the order of the tree
    w = _random_word(rng)
    t = RR.tones(G, np.frombuffer(w, np.uint8))
    tiny = (rng.random(79) * 0.3 + 0.3).astype(F32)                     # each below half an ulp of the huge term, together far above it
    planes = []
    for n_huge in (0, 14, 40, 64, 78):
        sig, noi = tiny.copy(), tiny[::-1].copy()
        sig[n_huge] = F32(3.0e7)
        noi[78 - n_huge] = F32(1.0e4)
        planes.append(dict(plane=plane_of_terms(2, 3, t, sig, noi), list=_cands([(2, 3)])))
    out.append(_case("huge_and_tiny", planes, [[(0, w)] for _ in planes]))
    # (e) the XOR reduction: the all-ones word, the encoder's densest rows alone, rows 64..90 alone (lanes 0..26), rows 0..63 alone
    dense = np.argsort(-G.sum(axis=1), kind="stable")[:6]
    words = [ALL_ONES] + [word_of_bits(np.eye(RR.K, dtype=np.uint8)[k]) for k in list(dense) + [63, 64, 90]]
    words += [word_of_bits(np.arange(RR.K) >= 64), word_of_bits(np.arange(RR.K) < 64)]
    ch = dict(plane=_noise_plane(rng, 32), list=_cands([(1, 2), (17, -3)]))
    out.append(_case("xor_reduction", [ch], [[(q & 1, wd) for q, wd in enumerate(words)]]))
    # (f) channels: 2, and 257 with empty channels first, last and in a row (the search crosses equal offsets)
    chs = [dict(plane=_noise_plane(rng, 32), list=_cands([(int(rng.integers(0, 18)), int(rng.integers(-20, 40)))])) for _ in range(2)]
    out.append(_case("channels_2", chs, [[(0, _random_word(rng)) for _ in range(3)], [(0, _random_word(rng)) for _ in range(2)]]))
    chs = [dict(plane=_noise_plane(rng, 32), list=_cands([(int(rng.integers(0, 18)), int(rng.integers(-20, 40))) for _ in range(2)])) for _ in range(257)]
    counts = [int(v) for v in rng.integers(0, 3, 257)]
    counts[0] = counts[1] = counts[256] = 0
    counts[100:140] = [0] * 40
    counts[2], counts[255] = 2, 1
    out.append(_case("channels_257", chs, [[(int(rng.integers(0, 2)), _random_word(rng)) for _ in range(k)] for k in counts]))
    # (g) a limit below the total: nothing is written past report lim; and a limit above it
    ch = dict(plane=_noise_plane(rng, 32), list=_cands([(4, 4)]))
    rs = [[(0, _random_word(rng)) for _ in range(6)]]
    out.append(_case("limit_below_total", [ch], rs, lim=5, n_total=9))
    out.append(_case("limit_above_total", [ch], rs, lim=11))
    return tuple(out)


def answer(case):
    """The report block the kernel must leave: uint32[4 * (lim + 8)], 0xAB beyond report min(n_total, lim)."""
    G = encoder(case["seed"])
    n = min(case["n_total"], case["lim"])
    rep = np.full(REP_WORDS * (case["lim"] + GUARD_RECS), AB, np.uint32)
    recs = case["records"][:n]
    planes = {100 + c: ch["plane"] for c, ch in enumerate(case["channels"])}
    lists = {100 + c: ch["list"] for c, ch in enumerate(case["channels"])}
    rep[:REP_WORDS * n] = RR.reports(G, planes, lists, recs).view(np.uint32)
    return rep


def write_cases(path, cs):
    with open(path, "wb") as f:
        f.write(b"RPK1" + struct.pack("<i", len(cs)))
        for case in cs:
            f.write(struct.pack("<3i", len(case["channels"]), case["n_total"], case["lim"]))
            f.write(enc_words(encoder(case["seed"])).tobytes())
            f.write(case["offsets"].tobytes())
            for ch in case["channels"]:
                assert ch["plane"].dtype == F32 and ch["plane"].shape[0] == RR.NHSYM and ch["list"].dtype == CAND
                f.write(struct.pack("<2i", ch["plane"].shape[1], len(ch["list"])))
                f.write(np.ascontiguousarray(ch["plane"]).tobytes())
                f.write(ch["list"].tobytes())
            f.write(case["records"][:min(case["n_total"], case["lim"])].tobytes())


def read_results(path, cs):
    w = np.fromfile(path, np.uint32)
    assert w[0] == int.from_bytes(b"RPR1", "little") and w[1] == len(cs)
    at, res = 2, []
    for case in cs:
        assert w[at] == case["lim"], case["name"]
        k = REP_WORDS * (case["lim"] + GUARD_RECS)
        res.append(w[at + 1:at + 1 + k])
        at += 1 + k
    assert at == len(w)
    return res


def build_check_program(out_dir):
    """Compile tests/report_kernel_check.hip with the product's flags (without -shared -fPIC) -> the program's path."""
    from cwsl_digi_amd import build as B
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc is needed to build the kernel's check program")
    exe = os.path.join(str(out_dir), "report_kernel_check")
    flags = [f for f in B.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "report_kernel_check.hip")
    subprocess.check_call([hipcc] + flags + ["-Wall", "-Werror", "-I", B.CSRC, src, "-o", exe])
    return exe


def first_difference(case, got, want):
    if np.array_equal(got, want):
        return ""
    g, w = got.reshape(-1, REP_WORDS), want.reshape(-1, REP_WORDS)
    p = int(np.nonzero((g != w).any(axis=1))[0][0])
    n = min(case["n_total"], case["lim"])
    what = f"report {p} of {n}" if p < n else f"guard report {p} (past the {n} that may be written)"
    return f"{case['name']}: {what}: {g[p].view(RR.REPORT_DTYPE)[0]} = {g[p].tobytes().hex()}, expected {w[p].view(RR.REPORT_DTYPE)[0]} = {w[p].tobytes().hex()}"
