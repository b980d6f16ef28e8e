"""Test helper: ft4_report_kernel (csrc/ft4soft_kernels.hpp) on frame spectra, sync records and decode records the test
writes -- the cases of tests/test_gpu_ft4_report_kernel.py, the file formats of tests/ft4_report_kernel_check.hip, and what the kernel must leave
in its report block, computed by tests/ft4_decode_reports_ref.py alone (oracle.ft4_downsample -> ft4_softbits_ref.symbol_spectra -> the report).
tests/test_ft4_report_kernel_inputs.py proves what the cases contain."""
import functools
import os
import struct
import subprocess

import numpy as np

import decodes_ref as DR
import ft4_decode_reports_ref as R4
import ft4_softbits_ref as S4
import ldpc_cases as LC
import report_kernel_cases as K8

F32 = np.float32
AB = 0xABABABAB
GUARD_RECS, HEAD_WORDS, REC_WORDS, REP_WORDS = 8, 4, 10, 4              # as in ft4_report_kernel_check.hip
SYNC4 = np.dtype([("f0_hz", F32), ("f1_hz", F32), ("dt_s", F32), ("sync", F32), ("ibest", np.int32), ("idf", np.int32), ("seg", np.int32), ("cand", np.int32)])
SEED = LC.SEEDS[0]
ALL_ONES = K8.ALL_ONES
NCX = 36289
F1_LO, F1_HI = 10.5, 4989.5                                             # ft4_refine_kernel keeps a record only for 10 < f1 < 4990
IBEST_LO, IBEST_HI = -349, 1017                                         # the fine search's reach around the coarse grid -344 .. 1012
HALF_TONE_HZ = 12000.0 / 576.0 / 2.0
BURST_AT, BURST_SYMBOLS = 3300, (0, 38, 39, 64, 102)                    # spectrum "burst": its loud symbol's first baseband sample; the symbol of a record it falls on
encoder, enc_words, word_of_bits = K8.encoder, K8.enc_words, K8.word_of_bits
CW_HZ, CW_IBEST = 1200.0, 320                                           # spectrum "cw": a codeword's transmission, tone 0 and first baseband sample
CW_WORD = word_of_bits(np.random.default_rng(77).integers(0, 2, 91))    # ... and its word


# ---- frame spectra --------------------------------------------------------------------------------------------------------------------------------------
def _spectrum_of(frame):
    from oracle import oracle as orc
    cx = np.array(orc.ft4_bigspec(frame), np.complex64)
    assert cx.shape == (NCX,)
    cx.setflags(write=False)
    return cx


@functools.lru_cache(maxsize=None)
def spectra():
    """The frame spectra the cases share, by name (their order is the file's).
    tx: four transmissions (600 / 1500 / 2600 / 3400 Hz) in noise; noise: noise alone; zero: all zero; burst: faint noise and ONE symbol's worth
    of a loud tone at 1000 Hz from baseband sample BURST_AT -- one huge term among small ones; carrier: one carrier half a tone spacing above
    1000 Hz, so that tones 0 and 1 are equally strong to 1 part in 10^4 at f1 = 1000."""
    tx, _ = S4.ft4_frame([(600.0, 0.5, 900.0, 11), (1500.0, 0.3, 700.0, 12), (2600.0, 0.6, 500.0, 13), (3400.0, 0.45, 1100.0, 14)], 300.0, 501)
    noise, _ = S4.ft4_frame([], 300.0, 502)
    rng = np.random.default_rng(503)
    x = rng.normal(0.0, 1.5, 90000)
    i0 = 18 * BURST_AT                                                  # 18 frame samples per baseband sample
    x[i0:i0 + 576] += 30000.0 * np.cos(2 * np.pi * 1000.0 * np.arange(576) / 12000.0)
    burst = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    carrier = np.rint(8000.0 * np.cos(2 * np.pi * (1000.0 + HALF_TONE_HZ) * np.arange(90000) / 12000.0)).astype(np.int16)
    # a codeword's transmission at CW_HZ, starting CW_IBEST baseband samples into the frame, in the same noise as "noise"
    y = np.random.default_rng(502).normal(0.0, 300.0, 90000)
    ph = S4._phase(R4.tones(encoder(SEED), np.frombuffer(CW_WORD, np.uint8)), CW_HZ, 576, 12000.0)
    y[18 * CW_IBEST:18 * CW_IBEST + len(ph)] += 600.0 * np.cos(ph)
    cw = np.clip(np.rint(y), -32768, 32767).astype(np.int16)
    return dict(tx=_spectrum_of(tx), noise=_spectrum_of(noise), zero=np.zeros(NCX, np.complex64), burst=_spectrum_of(burst), carrier=_spectrum_of(carrier),
                cw=_spectrum_of(cw))


SPECTRA = ("tx", "noise", "zero", "burst", "carrier", "cw")


# ---- hand-made basebands ---------------------------------------------------------------------------------------------------------------------------------
def baseband_of_amps(ibest, amps):
    """A baseband complex64[4032] whose symbol spectra, seen from ibest, are EXACTLY cs[n][q] = (amps[n][q], 0): symbol n carries the four samples
    x[8 j] = sum_q amps[n][q] / 4 * i^(q j) (j = 0..3) and zeros between them -- the symbol spectrum is then a 4-point transform at the table's
    exact cardinal points.  amps: float32[103, 4] of values whose quarter sums are exact in float32; samples outside 0..4031 are dropped."""
    amps = np.asarray(amps, np.float64).reshape(S4.NN, 4)
    cb = np.zeros(S4.NP, np.complex128)
    for n in range(S4.NN):
        for j in range(4):
            m = int(ibest) + 32 * n + 8 * j
            if 0 <= m < S4.NP:
                cb[m] = sum(amps[n, q] / 4.0 * (1j ** ((q * j) % 4)) for q in range(4))
    out = cb.astype(np.complex64)
    assert np.array_equal(out.astype(np.complex128), cb)
    return out


# ---- channels ---------------------------------------------------------------------------------------------------------------------------------------------
def _channel(spectrum, nrec, recs, cap=None, cnt=None):
    """nrec: records per candidate; recs: [(f1_hz, ibest)] of the records in compacted order.  -> dict(spectrum, cap, cnt, nrec int32[cap],
    rec SYNC4[cap, 3], sync: the compacted records as dicts)."""
    nrec = np.asarray(nrec, np.int32)
    cap = len(nrec) if cap is None else cap
    full = np.zeros(cap, np.int32)
    full[:len(nrec)] = nrec
    rec = np.zeros((cap, 3), SYNC4)
    rec["f1_hz"], rec["ibest"] = F32(777.0), 7                          # (slots without a record: never read)
    sync, q = [], 0
    for k, v in enumerate(nrec):
        for r in range(int(v)):
            f1, ib = recs[q]
            rec[k, r] = (F32(f1) - F32(1), F32(f1), F32(ib) / F32(666.67) - F32(0.5), 2.0, ib, 1, r + 1, k)
            sync.append(dict(f1_hz=F32(f1), ibest=int(ib)))
            q += 1
    assert q == len(recs)
    return dict(spectrum=spectrum, cap=cap, cnt=len(nrec) if cnt is None else cnt, nrec=full, rec=rec, sync=sync)


def _decode(ch_id, entry, word):
    r = np.zeros((), DR.DECODE_DTYPE)
    r["ch_id"], r["entry"], r["bits"] = ch_id, entry, np.frombuffer(word, np.uint8)
    r["ndup"] = 1
    return r


def _random_word(rng):
    return word_of_bits(rng.integers(0, 2, 91))


def _case(name, channels, per_channel_records, seed=SEED, lim=None, n_total=None):
    """per_channel_records: [[(entry, word)]] -- the records of channel c in order.  lim None: everything."""
    recs, offsets = [], []
    for c, rs in enumerate(per_channel_records):
        offsets.append(len(recs))
        recs += [_decode(100 + c, e, w) for e, w in rs]
    recs = np.array(recs, DR.DECODE_DTYPE) if recs else np.zeros(0, DR.DECODE_DTYPE)
    total = len(recs) if n_total is None else n_total
    return dict(name=name, seed=seed, channels=channels, offsets=np.array(offsets, np.uint32), records=recs, n_total=total,
                lim=len(recs) if lim is None else lim)


TX = ((600.0, 333), (1500.0, 200), (2600.0, 400), (3400.0, 300))       # (f1_hz, ibest) of spectrum "tx"'s transmissions: 0.5 s + start, 666.67 samples a second


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20264)
    G = encoder(SEED)
    out = []
    some = lambda n: [(float(rng.uniform(250, 3800)), int(rng.integers(-300, 1000))) for _ in range(n)]
    # (a) 1, 2, 3, 5 decodes of one channel
    for nd in (1, 2, 3, 5):
        ch = _channel("tx", [1, 2, 0, 3, 1], list(TX) + some(3))
        out.append(_case(f"decodes_{nd}", [ch], [[(int(rng.integers(0, 7)), _random_word(rng)) for _ in range(nd)]]))
    # (b) 600 candidates with nrec 0..3: the prefix crosses the passes of 256 and ends in the last slot; an entry in a slot 3k + 2
    nrec = rng.integers(0, 4, 600)
    nrec[255], nrec[256], nrec[511], nrec[512], nrec[599], nrec[0] = 3, 2, 1, 3, 3, 0
    ch = _channel("tx", nrec, some(int(nrec.sum())))
    pre = np.concatenate([[0], np.cumsum(nrec)])
    entries = [int(pre[255]) + 2, int(pre[256]), int(pre[256]) + 1, int(pre[511]), int(pre[512]) + 2, int(pre[600]) - 1, 0, int(pre[300]), int(pre[599])]
    out.append(_case("candidates_600", [ch], [[(e, _random_word(rng)) for e in entries]]))
    # (c) f1_hz at both ends of the band, ibest at both extremes
    ch = _channel("noise", [3, 3], [(F1_LO, 100), (F1_HI, 100), (1234.5, IBEST_LO), (1234.5, IBEST_HI), (F1_LO, IBEST_LO), (F1_HI, IBEST_HI)])
    out.append(_case("band_and_time_edges", [ch], [[(e, _random_word(rng)) for e in range(6)]]))
    # (d) tones 0 and 1 equally strong to 1 part in 10^4; the zero spectrum: every first maximum a tie
    ch = _channel("carrier", [2], [(1000.0, 50), (1000.0 + 2 * HALF_TONE_HZ, 51)])
    out.append(_case("half_tone_carrier", [ch], [[(0, _random_word(rng)), (1, _random_word(rng)), (0, ALL_ONES)]]))
    ch = _channel("zero", [1, 1], [(1000.0, 0), (2000.0, 500)])
    out.append(_case("zero_spectrum", [ch], [[(0, word_of_bits(np.zeros(91, np.uint8) + (np.arange(91) == 5))), (1, _random_word(rng)), (1, ALL_ONES)]]))
    # (e) one huge term among small ones, at symbols 0, 38, 39, 64 and 102 of the record (lanes 0, 38 / 39: the last with two terms, the first
    # with one, 0 again as term 64, and 38 as term 102)
    ch = _channel("burst", [3, 2], [(1000.0, BURST_AT - 32 * n) for n in BURST_SYMBOLS])
    w = _random_word(rng)
    out.append(_case("huge_and_small", [ch], [[(e, w) for e in range(5)]]))
    # (f) the XOR reduction: the all-ones word, the encoder's densest rows alone, rows 64..90 alone (lanes 0..26), rows 0..63 alone
    dense = np.argsort(-G.sum(axis=1), kind="stable")[:6]
    words = [ALL_ONES] + [word_of_bits(np.eye(91, dtype=np.uint8)[k]) for k in list(dense) + [63, 64, 90]]
    words += [word_of_bits(np.arange(91) >= 64), word_of_bits(np.arange(91) < 64)]
    ch = _channel("tx", [2], [TX[0], TX[3]])
    out.append(_case("xor_reduction", [ch], [[(q & 1, wd) for q, wd in enumerate(words)]]))
    # (g) channels: 2, and 257 with empty channels first, last and 40 in a row (the search crosses equal offsets); a cnt above and below cap
    chs = [_channel("tx", [1, 1], [TX[0], TX[1]], cap=4, cnt=9), _channel("noise", [0, 2, 1], some(3), cap=5, cnt=3)]
    out.append(_case("channels_2", chs, [[(1, _random_word(rng)), (0, _random_word(rng)), (1, _random_word(rng))], [(2, _random_word(rng)), (0, _random_word(rng))]]))
    chs = [_channel(SPECTRA[int(rng.integers(0, 2))], [1, 0, 2], some(3)) for _ in range(257)]
    counts = [int(v) for v in rng.integers(0, 2, 257)]
    counts[0] = counts[1] = counts[256] = 0
    counts[100:140] = [0] * 40
    counts[2], counts[255] = 2, 1
    out.append(_case("channels_257", chs, [[(int(rng.integers(0, 3)), _random_word(rng)) for _ in range(k)] for k in counts]))
    # (i) the word that was sent, at its place, one sample early and at the wrong place; another word at its place
    ch = _channel("cw", [3, 1], [(CW_HZ, CW_IBEST), (CW_HZ, CW_IBEST - 1), (CW_HZ + 40.0, CW_IBEST), (CW_HZ, CW_IBEST)])
    out.append(_case("sent_word", [ch], [[(0, CW_WORD), (1, CW_WORD), (2, CW_WORD), (3, _random_word(rng))]]))
    # (h) a limit below the total: nothing is written past report lim; and a limit above it
    ch = _channel("tx", [1], [TX[2]])
    rs = [[(0, _random_word(rng)) for _ in range(4)]]
    out.append(_case("limit_below_total", [ch], rs, lim=3, n_total=7))
    out.append(_case("limit_above_total", [ch], rs, lim=9))
    return tuple(out)


def answer(case):
    """The report block the kernel must leave: uint32[4 * (lim + 8)], 0xAB beyond report min(n_total, lim)."""
    from oracle import oracle as orc
    G = encoder(case["seed"])
    n = min(case["n_total"], case["lim"])
    rep = np.full(REP_WORDS * (case["lim"] + GUARD_RECS), AB, np.uint32)
    recs = case["records"][:n]
    sp = spectra()
    cx = {100 + c: sp[ch["spectrum"]] for c, ch in enumerate(case["channels"])}
    sync = {100 + c: ch["sync"] for c, ch in enumerate(case["channels"])}
    rep[:REP_WORDS * n] = R4.reports(orc, G, cx, sync, recs).view(np.uint32)
    return rep


def write_cases(path, cs):
    sp = spectra()
    with open(path, "wb") as f:
        f.write(b"F4K1" + struct.pack("<2i", len(cs), len(SPECTRA)))
        for name in SPECTRA:
            f.write(np.ascontiguousarray(sp[name], np.complex64).tobytes())
        for case in cs:
            f.write(struct.pack("<3i", len(case["channels"]), case["n_total"], case["lim"]))
            f.write(enc_words(encoder(case["seed"])).tobytes())
            f.write(case["offsets"].tobytes())
            for ch in case["channels"]:
                assert ch["nrec"].dtype == np.int32 and ch["rec"].dtype == SYNC4 and ch["rec"].shape == (ch["cap"], 3)
                f.write(struct.pack("<3i", SPECTRA.index(ch["spectrum"]), ch["cap"], ch["cnt"]))
                f.write(ch["nrec"].tobytes())
                f.write(ch["rec"].tobytes())
            f.write(case["records"][:min(case["n_total"], case["lim"])].tobytes())


def read_results(path, cs):
    w = np.fromfile(path, np.uint32)
    assert w[0] == int.from_bytes(b"F4R1", "little") and w[1] == len(cs)
    at, res = 2, []
    for case in cs:
        assert w[at] == case["lim"], case["name"]
        k = REP_WORDS * (case["lim"] + GUARD_RECS)
        res.append(w[at + 1:at + 1 + k])
        at += 1 + k
    assert at == len(w)
    return res


def build_check_program(out_dir):
    """Compile tests/ft4_report_kernel_check.hip with the product's flags (without -shared -fPIC) -> the program's path."""
    from cwsl_digi_amd import build as B
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc is needed to build the kernel's check program")
    exe = os.path.join(str(out_dir), "ft4_report_kernel_check")
    flags = [f for f in B.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ft4_report_kernel_check.hip")
    subprocess.check_call([hipcc] + flags + ["-Wall", "-Werror", "-I", B.CSRC, src, "-o", exe])
    return exe


def _same_word(g, w):
    """Report words equal -- xsig / xnoise (words 1, 2) also when both are NaN: the sign of a generated NaN differs between hosts and the GPU."""
    if np.array_equal(g, w):
        return True
    if g[0] != w[0] or g[3] != w[3]:
        return False
    gf, wf = g[1:3].view(F32), w[1:3].view(F32)
    return all(a == b or (np.isnan(x) and np.isnan(y)) for a, b, x, y in zip(g[1:3], w[1:3], gf, wf))


def first_difference(case, got, want):
    if np.array_equal(got, want):
        return ""
    g, w = got.reshape(-1, REP_WORDS), want.reshape(-1, REP_WORDS)
    n = min(case["n_total"], case["lim"])
    bad = [p for p in range(len(g)) if not (_same_word(g[p], w[p]) if p < n else np.array_equal(g[p], w[p]))]
    if not bad:
        return ""
    p = bad[0]
    what = f"report {p} of {n}" if p < n else f"guard report {p} (past the {n} that may be written)"
    return f"{case['name']}: {what}: {g[p].view(R4.REPORT_DTYPE)[0]} = {g[p].tobytes().hex()}, expected {w[p].view(R4.REPORT_DTYPE)[0]} = {w[p].tobytes().hex()}"
