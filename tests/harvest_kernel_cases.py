"""Test helper: decode_harvest_kernel (csrc/harvest_kernels.hpp) on records the test writes -- the cases of tests/test_gpu_harvest_kernel.py, the
file formats of tests/harvest_kernel_check.hip, and what the kernel must leave in its three blocks, computed by tests/decodes_ref.py alone.

No radio slot fills a channel with 300 words, so the carries of the kernel (256 slots, 256 listed words, 256 survivors and 256 channels per
pass) are reached with synthetic records only: seeded random arrays in the records' numpy dtypes, handed to the kernel through its descriptor.
A case is dict(name, ft4, max_out, channels); a channel is dict(ch_id, cap, cnt, list, nrec, msg, osd, osd_null) with arrays of `cap` entries
(FT4: [cap][3] slots).  What lies beyond the count, in the slots of an FT4 candidate beyond its nrec, or in the fields next to a zero crc_ok is
filled with plausible records ON PURPOSE: the kernel must not look there.  tests/test_harvest_kernel_inputs.py proves what the cases contain."""
import functools
import os
import struct
import subprocess

import numpy as np

import decodes_ref as DR
import ft4_decode_cases as D4
import ft4_osd_cases as X4
import ldpc_ref as R
import osd_ref as O
import record_race_cases as RC

SEED = 20261
MAXCAND = 600                                                           # SYNC_MAXCAND_CAP
NT = 256                                                                # HARVEST_NT: slots, listed words, survivors and channels per pass
GUARD_RECS, GUARD_WORDS, HEAD_WORDS, REC_WORDS = 8, 8, 4, 10            # as in harvest_kernel_check.hip
AB = 0xABABABAB
MSG, OSD, MSG4, OSD4, CAND, SYNC4 = R.MSG_DTYPE, O.OSD_DTYPE, D4.MSG4_DTYPE, X4.OSD4_DTYPE, RC.CAND_DTYPE, RC.SYNC4_DTYPE


def _rng(*key):
    return np.random.default_rng([SEED] + [int(k) for k in key])


def pool(rng, n):
    """n distinct non-zero words, the five padding bits of byte 11 zero."""
    w = rng.integers(0, 256, (n, 12), dtype=np.uint8)
    w[:, 11] &= 0xE0
    assert len({bytes(x) for x in w}) == n and not any(DR.all_zero_word(x) for x in w)
    return w


# ---- records --------------------------------------------------------------------------------------------------------------------------------------
def noise_msg(rng, shape):
    """Decode records without a word: crc_ok 0 and everything else as arbitrary as a record allows (bits, pad_ included)."""
    m = np.zeros(shape, MSG)
    m["bits"] = rng.integers(0, 256, m["bits"].shape, dtype=np.uint8)
    m["iters"], m["nbad"], m["nharderr"] = (rng.integers(0, 175, shape) for _ in range(3))
    m["pad_"] = rng.integers(0, 256, shape)
    return m


def noise_osd(rng, shape):
    o = np.zeros(shape, OSD)
    o["bits"] = rng.integers(0, 256, o["bits"].shape, dtype=np.uint8)
    o["dmin"] = rng.uniform(0.5, 90.0, shape).astype(np.float32)
    o["nharderr"], o["nskip"] = rng.integers(0, 175, shape), rng.integers(0, 40, shape)
    o["how"] = rng.integers(0, 4, shape)
    o["flip"] = rng.integers(0, 91, o["flip"].shape)
    return o


def set_word(rec, at, word, nharderr, crc_ok=1):
    """rec[at] (a decode or an OSD record) carries `word` with crc_ok."""
    rec["bits"][at], rec["nharderr"][at], rec["crc_ok"][at] = word, nharderr, crc_ok


def cand_list(rng, cap):
    c = np.zeros(cap, CAND)
    c["freq_bin"], c["time_step"] = rng.integers(64, 960, cap), rng.integers(-62, 63, cap)
    c["sync"], c["freq_hz"], c["dt_s"] = (rng.uniform(lo, hi, cap).astype(np.float32) for lo, hi in ((1.0, 40.0), (200.0, 3000.0), (-2.5, 2.5)))
    return c


def sync4_list(rng, cap):
    s = np.zeros((cap, 3), SYNC4)
    for name, lo, hi in (("f0_hz", 200.0, 3000.0), ("f1_hz", 200.0, 3000.0), ("dt_s", -1.0, 1.0), ("sync", 1.0, 40.0)):
        s[name] = rng.uniform(lo, hi, (cap, 3)).astype(np.float32)
    for name in ("ibest", "idf", "seg", "cand"):
        s[name] = rng.integers(0, 600, (cap, 3))
    assert (s["f0_hz"] != s["f1_hz"]).all()
    return s


def ft8_channel(rng, ch_id, cap, cnt, bp=(), osd=(), osd_null=False, poison=None):
    """An FT8 channel: bp / osd: (entry, word, nharderr[, crc_ok]) that carry a word.  poison: words for BP records of the entries from the count
    on, which the kernel must not read."""
    ch = dict(ch_id=ch_id, cap=cap, cnt=cnt, list=cand_list(rng, cap), nrec=None, msg=noise_msg(rng, cap), osd=noise_osd(rng, cap), osd_null=osd_null)
    for rec, words in ((ch["msg"], bp), (ch["osd"], osd)):
        for q, word, nh, *crc in words:
            set_word(rec, q, word, nh, *crc)
    if poison is not None:
        for q in range(max(0, min(cnt, cap)), cap):
            set_word(ch["msg"], q, poison[q % len(poison)], 1)
    return ch


def ft4_channel(rng, ch_id, cap, cnt, nrec, bp=(), osd=(), osd_null=False):
    """An FT4 channel: bp / osd: (candidate, record, set, word, nharderr) that carry a word."""
    ch = dict(ch_id=ch_id, cap=cap, cnt=cnt, list=sync4_list(rng, cap), nrec=np.asarray(nrec, np.int32), osd_null=osd_null,
              msg=np.zeros((cap, 3), MSG4), osd=np.zeros((cap, 3), OSD4))
    assert ch["nrec"].shape == (cap,)
    ch["msg"]["set"], ch["osd"]["set"] = noise_msg(rng, (cap, 3, 3)), noise_osd(rng, (cap, 3, 3))
    for rec, words in ((ch["msg"], bp), (ch["osd"], osd)):
        for k, r, s, word, nh in words:
            set_word(rec["set"], (k, r, s), word, nh)
    return ch


# ---- what the kernel must leave -------------------------------------------------------------------------------------------------------------------
def n_listed(ch):
    """Entries of the list the contract speaks of: all min(count, max_cand) of them, at most 600."""
    return max(0, min(int(ch["cnt"]), int(ch["cap"]), MAXCAND))


def existing_slots(ch):
    """FT4: the (candidate, record) pairs that exist, in ascending slot order -- the order in which cwslg_fetch_ft4_sync compacts the records."""
    return [(k, r) for k in range(n_listed(ch)) for r in range(int(ch["nrec"][k]))]


def channel_input(case, ch):
    """decodes_ref's input for one channel: (ch_id, where, msg, osd) of its entries."""
    osd = None if ch["osd_null"] else ch["osd"]
    if not case["ft4"]:
        n = n_listed(ch)
        where = [(c["freq_hz"], c["dt_s"], c["sync"]) for c in ch["list"][:n]]
        return ch["ch_id"], where, ch["msg"][:n], None if osd is None else osd[:n]
    at = existing_slots(ch)
    kk, rr = np.array([k for k, _ in at], np.intp), np.array([r for _, r in at], np.intp)
    where = [(s["f1_hz"], s["dt_s"], s["sync"]) for s in ch["list"][kk, rr]]
    return ch["ch_id"], where, ch["msg"][kk, rr], None if osd is None else osd[kk, rr]


def n_words(case, ch):
    """Entries of the channel that carry a word (before de-duplication): what the kernel lists."""
    _, _, msg, osd = channel_input(case, ch)
    ws = ((DR._word_ft4 if case["ft4"] else DR._word_ft8)(msg[q], None if osd is None else osd[q]) for q in range(len(msg)))
    return sum(1 for w in ws if w is not None and not DR.all_zero_word(w[2]))


def answer(case):
    """(records, counts) of a case without the cut at max_out: the decodes of all channels in output order, and the decodes per channel in
    descriptor order."""
    mode = "FT4" if case["ft4"] else "FT8"
    inputs = [channel_input(case, ch) for ch in case["channels"]]
    assert [i[0] for i in inputs] == sorted(i[0] for i in inputs)       # descriptor order is ascending ch_id, as the library builds it
    counts = [len(DR.channel_decodes(mode, *i)) for i in inputs]
    recs, n_total = DR.decodes(mode, inputs)
    assert n_total == sum(counts) == len(recs)
    return recs, counts


def blocks(case, recs, counts):
    """The three blocks after the launches, as uint32 arrays: counts and offsets (n_chan + 8 words), out (4 + 10 (max_out + 8) words)."""
    n_chan, max_out = len(case["channels"]), case["max_out"]
    c = np.full(n_chan + GUARD_WORDS, AB, np.uint32)
    o = c.copy()
    c[:n_chan] = counts
    o[:n_chan] = np.concatenate([[0], np.cumsum(counts)[:-1]])
    out = np.full(HEAD_WORDS + REC_WORDS * (max_out + GUARD_RECS), AB, np.uint32)
    out[0] = len(recs)
    n = min(len(recs), max_out)
    out[HEAD_WORDS:HEAD_WORDS + REC_WORDS * n] = recs[:n].view(np.uint32)
    return c, o, out


# ---- the files of harvest_kernel_check -------------------------------------------------------------------------------------------------------------
def write_cases(path, cases):
    with open(path, "wb") as f:
        f.write(b"HVK1" + struct.pack("<i", len(cases)))
        for case in cases:
            f.write(struct.pack("<3i", int(case["ft4"]), case["max_out"], len(case["channels"])))
            for ch in case["channels"]:
                cap, slots = ch["cap"], (ch["cap"], 3) if case["ft4"] else (ch["cap"],)
                f.write(struct.pack("<4i", ch["ch_id"], cap, ch["cnt"], int(ch["osd_null"])))
                for name, dtype in (("list", SYNC4 if case["ft4"] else CAND), ("nrec", np.int32), ("msg", MSG4 if case["ft4"] else MSG),
                                    ("osd", OSD4 if case["ft4"] else OSD)):
                    if ch[name] is None:
                        assert name == "nrec" and not case["ft4"]
                        continue
                    assert ch[name].dtype == dtype and ch[name].shape == ((cap,) if name == "nrec" else slots), (case["name"], name)
                    f.write(np.ascontiguousarray(ch[name]).tobytes())


def read_results(path, cases):
    """[(counts, offsets, out)] per case, uint32 arrays."""
    w = np.fromfile(path, np.uint32)
    assert w[0] == int.from_bytes(b"HVR1", "little") and w[1] == len(cases), (w[:2], len(cases))
    at, res = 2, []
    for case in cases:
        n_chan, max_out = len(case["channels"]), case["max_out"]
        assert (w[at], w[at + 1]) == (n_chan, max_out), case["name"]
        nc, no = n_chan + GUARD_WORDS, HEAD_WORDS + REC_WORDS * (max_out + GUARD_RECS)
        res.append((w[at + 2:at + 2 + nc], w[at + 2 + nc:at + 2 + 2 * nc], w[at + 2 + 2 * nc:at + 2 + 2 * nc + no]))
        at += 2 + 2 * nc + no
    assert at == len(w)
    return res


def build_check_program(out_dir):
    """Compile tests/harvest_kernel_check.hip with the product's flags (without -shared -fPIC) -> the program's path."""
    from cwsl_digi_amd import build as B
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc is needed to build the kernel's check program")
    exe = os.path.join(str(out_dir), "harvest_kernel_check")
    flags = [f for f in B.HIPCC_FLAGS if f not in ("-shared", "-fPIC")]
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "harvest_kernel_check.hip")
    subprocess.check_call([hipcc] + flags + ["-Wall", "-Werror", "-I", B.CSRC, src, "-o", exe])
    return exe


def first_difference(case, got, want):
    """'' if the blocks (counts, offsets, out) are equal, else a description that names the case and the first differing word or record."""
    for name, g, w in zip(("counts", "offsets"), got, want):
        if not np.array_equal(g, w):
            i = int(np.nonzero(g != w)[0][0])
            return f"{case['name']}: {name}[{i}] = {int(g[i]):#x}, expected {int(w[i]):#x} ({len(case['channels'])} channels)"
    g, w = got[2], want[2]
    if np.array_equal(g, w):
        return ""
    if not np.array_equal(g[:HEAD_WORDS], w[:HEAD_WORDS]):
        return f"{case['name']}: head {[hex(int(v)) for v in g[:HEAD_WORDS]]}, expected {[hex(int(v)) for v in w[:HEAD_WORDS]]}"
    gr, wr = g[HEAD_WORDS:].reshape(-1, REC_WORDS), w[HEAD_WORDS:].reshape(-1, REC_WORDS)
    i = int(np.nonzero((gr != wr).any(axis=1))[0][0])
    n = min(int(w[0]), case["max_out"])
    what = f"record {i} of {n}" if i < n else f"guard record {i} (past the {n} that may be written)"
    return f"{case['name']}: {what}: {gr[i].view(DR.DECODE_DTYPE)[0]} = {gr[i].tobytes().hex()}, expected {wr[i].view(DR.DECODE_DTYPE)[0]} = {wr[i].tobytes().hex()}"


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------------
def _case(name, ft4, channels, max_out=None, literal=None):
    """max_out None: eight more than the total, so that everything comes out.  literal: the expected records written out by hand."""
    case = dict(name=name, ft4=ft4, channels=channels, max_out=0, literal=literal)
    case["max_out"] = len(answer(case)[0]) + GUARD_RECS if max_out is None else max_out
    return case


def lit(ch_id, entry, by_osd, set_, word, freq_hz, dt_s, sync, dmin, nharderr, ndup):
    """One expected record from explicit values."""
    r = np.zeros((), DR.DECODE_DTYPE)
    r["ch_id"], r["entry"], r["by_osd"], r["set"], r["bits"] = ch_id, entry, by_osd, set_, word
    r["freq_hz"], r["dt_s"], r["sync"], r["dmin"], r["nharderr"], r["ndup"] = freq_hz, dt_s, sync, dmin, nharderr, ndup
    return r


def _lit8(ch, entry, by_osd, word, nharderr, ndup):
    c = ch["list"][entry]
    return lit(ch["ch_id"], entry, by_osd, 0, word, c["freq_hz"], c["dt_s"], c["sync"], ch["osd"]["dmin"][entry] if by_osd else 0.0, nharderr, ndup)


def _lit4(ch, entry, k, r, by_osd, s, word, nharderr, ndup):
    c = ch["list"][k, r]
    return lit(ch["ch_id"], entry, by_osd, s, word, c["f1_hz"], c["dt_s"], c["sync"], ch["osd"]["set"]["dmin"][k, r, s] if by_osd else 0.0, nharderr, ndup)


FT8_COUNTS = ((600, 0), (600, -1), (600, 1), (600, 255), (600, 256), (600, 257), (600, 600), (600, 700), (5, 9))      # (cap, cnt)


def ft8_distinct():
    """One channel, every entry a distinct BP word (the entries from the count on too): slots = words = survivors = min(cnt, cap)."""
    out = []
    for cap, cnt in FT8_COUNTS:
        rng = _rng(1, cap, cnt + 1)
        words = pool(rng, cap)
        bp = [(q, words[q], int(rng.integers(0, 175))) for q in range(cap)]
        out.append(_case(f"ft8_distinct_cap{cap}_cnt{cnt}", 0, [ft8_channel(rng, 5, cap, cnt, bp=bp)]))
    return out


@functools.lru_cache(maxsize=None)
def _crowded_channel(osd_null):
    rng = _rng(2)
    words = pool(rng, 400)
    bp = [(q, words[rng.integers(400)], int(rng.integers(0, 175))) for q in range(600) if rng.random() < 0.5]
    osd = [(q, words[rng.integers(400)], int(rng.integers(0, 175))) for q in range(600) if rng.random() < 0.4]
    return ft8_channel(rng, 2, 600, 600, bp=bp, osd=osd, osd_null=osd_null)


def ft8_crowded():
    """600 entries on a pool of 400 words, BP on about half and OSD on about 40 % of them: more than 256 listed words and more than 256
    survivors; and the same records with the descriptor's osd null."""
    out = [_case("ft8_crowded", 0, [_crowded_channel(False)]), _case("ft8_crowded_osd_null", 0, [_crowded_channel(True)])]
    assert n_words(out[0], out[0]["channels"][0]) > NT and len(answer(out[0])[0]) > NT
    return out


def ft8_one_word():
    """600 entries, one word.  By OSD but for the BP entry 599, which wins; and all by BP with the fewest hard errors at entries 300 and 511, of
    which 300 wins."""
    rng = _rng(3)
    w = pool(rng, 1)[0]
    a = ft8_channel(rng, 0, 600, 600, bp=[(599, w, 80)], osd=[(q, w, int(rng.integers(0, 60))) for q in range(599)])
    b = ft8_channel(rng, 0, 600, 600, bp=[(q, w, 2 if q in (300, 511) else int(rng.integers(3, 175))) for q in range(600)])
    return [_case("ft8_one_word_bp_last", 0, [a], literal=[_lit8(a, 599, 0, w, 80, 600)]),
            _case("ft8_one_word_all_bp", 0, [b], literal=[_lit8(b, 300, 0, w, 2, 600)])]


def ft8_rank_across_passes():
    """One word on entry 0 (OSD, 0 hard errors), entry 2 (BP, 9) and entry 580 (BP, 3): entry 580 is reported, in its own place among the others."""
    rng = _rng(4)
    w = pool(rng, 7)
    others = [(1, w[1], 7), (100, w[2], 0), (300, w[3], 174), (579, w[4], 20), (581, w[5], 21), (599, w[6], 1)]
    ch = ft8_channel(rng, 9, 600, 600, bp=[(2, w[0], 9), (580, w[0], 3)] + others, osd=[(0, w[0], 0)])
    literal = sorted([_lit8(ch, q, 0, word, nh, 1) for q, word, nh in others] + [_lit8(ch, 580, 0, w[0], 3, 3)], key=lambda r: int(r["entry"]))
    return [_case("ft8_rank_across_passes", 0, [ch], literal=literal)]


def ft8_keys():
    """Words that differ in one of the three key words only stay apart (and so do words that differ in a padding bit: the contract compares
    bits[12]); zero words, zero crc_ok next to other non-zero bytes, and crc_ok = 0x80."""
    rng = _rng(5)
    b = pool(rng, 1)[0]
    flip = lambda byte, bit: np.concatenate([b[:byte], [b[byte] ^ bit], b[byte + 1:]]).astype(np.uint8)
    w1, w2, w3, wp = flip(1, 0x10), flip(5, 0x01), flip(11, 0x20), flip(11, 0x01)
    ch = ft8_channel(rng, 3, 8, 6, bp=[(0, b, 10), (1, w1, 11), (2, w2, 12), (3, w3, 13), (4, b, 14), (5, wp, 15)], poison=pool(rng, 2))
    bits = _case("ft8_keys_one_bit", 0, [ch], literal=[_lit8(ch, 0, 0, b, 10, 2), _lit8(ch, 1, 0, w1, 11, 1), _lit8(ch, 2, 0, w2, 12, 1),
                                                       _lit8(ch, 3, 0, w3, 13, 1), _lit8(ch, 5, 0, wp, 15, 1)])
    p = pool(rng, 5)
    zero, zero_pad = np.zeros(12, np.uint8), np.array([0] * 11 + [0x1F], np.uint8)
    ch = ft8_channel(rng, 4, 8, 8, bp=[(0, zero_pad, 0), (2, zero, 0), (4, p[3], 17, 0x80), (6, p[3], 5)],
                     osd=[(1, zero_pad, 0), (2, p[0], 3), (5, p[4], 40, 0x80)])
    ch["msg"]["bits"][3], ch["msg"]["pad_"][3] = p[1], 0xFF             # crc_ok 0 beside pad_ 0xff
    ch["osd"]["bits"][3], ch["osd"]["how"][3], ch["osd"]["flip"][3] = p[2], 3, (7, 9)      # OSD crc_ok 0 beside how and flip
    assert not ch["msg"]["crc_ok"][[1, 3, 5, 7]].any() and not ch["osd"]["crc_ok"][[0, 3, 4, 6, 7]].any()
    flags = _case("ft8_keys_zero_words_and_flags", 0, [ch], literal=[_lit8(ch, 5, 1, p[4], 40, 1), _lit8(ch, 6, 0, p[3], 5, 2)])
    return [bits, flags]


FT4_RUN = (170, 270)                                                    # candidates without a record: slots 510..809 hold the whole pass 512..767


@functools.lru_cache(maxsize=None)
def _ft4_crowded_channel(osd_null):
    rng = _rng(6)
    words = pool(rng, 500)
    nrec = rng.integers(0, 4, 600)
    nrec[FT4_RUN[0]:FT4_RUN[1]] = 0
    # EVERY slot, existing or not, holds BP and OSD records with crc_ok: about 25 % and 30 % per set
    bp = [(k, r, s, words[rng.integers(500)], int(rng.integers(0, 175))) for k in range(600) for r in range(3) for s in range(3) if rng.random() < 0.25]
    osd = [(k, r, s, words[rng.integers(500)], int(rng.integers(0, 175))) for k in range(600) for r in range(3) for s in range(3) if rng.random() < 0.30]
    for k in range(600):                                                # and a slot that does not exist holds both for certain
        for r in range(int(nrec[k]), 3):
            bp.append((k, r, int(rng.integers(3)), words[rng.integers(500)], int(rng.integers(0, 175))))
            osd.append((k, r, int(rng.integers(3)), words[rng.integers(500)], int(rng.integers(0, 175))))
    return ft4_channel(rng, 6, 600, 600, nrec, bp=bp, osd=osd, osd_null=osd_null)


def ft4_crowded():
    """cap 600, cnt 600, nrec in 0..3 with a whole 256-slot pass of candidates without a record; every slot that does not exist is poisoned."""
    out = [_case("ft4_crowded", 1, [_ft4_crowded_channel(False)]), _case("ft4_crowded_osd_null", 1, [_ft4_crowded_channel(True)])]
    ch, recs = out[0]["channels"][0], answer(out[0])[0]
    assert len(existing_slots(ch)) > NT and n_words(out[0], ch) > NT and len(recs) > NT
    assert all(set(recs["set"][recs["by_osd"] == by]) == {0, 1, 2} for by in (0, 1))
    return out


def ft4_small():
    """cnt 1 with nrec 0, 1 and 3 (the candidate beyond the count and the slots beyond nrec poisoned); cnt 86 with all nrec 3: 258 slots, the
    third record of candidate 85 in the second pass."""
    out = []
    for nrec in (0, 1, 3):
        rng = _rng(7, nrec)
        w = pool(rng, 9)
        bp = [(k, r, 1, w[3 * k + r], 10 + 3 * k + r) for k in range(2) for r in range(3)]       # every slot of both candidates: a distinct BP word of set 1
        osd = [(0, 0, 0, w[6], 1)]                                                               # shadowed by BP
        ch = ft4_channel(rng, 8, 2, 1, [nrec, 3], bp=bp, osd=osd)
        out.append(_case(f"ft4_cnt1_nrec{nrec}", 1, [ch], literal=[_lit4(ch, r, 0, r, 0, 1, w[r], 10 + r, 1) for r in range(nrec)]))
    rng = _rng(7, 86)
    w = pool(rng, 4)
    # slot 0: BP set 1; slot 3 = (1, 0): OSD set 2 of w[1]; slot 255 = (85, 0): OSD set 2; slot 256 = (85, 1): BP set 2 under an OSD set 0;
    # slot 257 = (85, 2): BP set 0 of w[1], which beats slot 3's OSD
    ch = ft4_channel(rng, 8, 86, 86, [3] * 86, bp=[(0, 0, 1, w[0], 30), (85, 1, 2, w[3], 33), (85, 2, 0, w[1], 90)],
                     osd=[(1, 0, 2, w[1], 2), (85, 0, 2, w[2], 50), (85, 1, 0, w[0], 0)])
    literal = [_lit4(ch, 0, 0, 0, 0, 1, w[0], 30, 1), _lit4(ch, 255, 85, 0, 1, 2, w[2], 50, 1), _lit4(ch, 256, 85, 1, 0, 2, w[3], 33, 1),
               _lit4(ch, 257, 85, 2, 0, 0, w[1], 90, 2)]
    out.append(_case("ft4_cnt86_nrec3", 1, [ch], literal=literal))
    return out


N_CHANNELS = (1, 255, 256, 257, 600)
ZERO_RUNS = ((96, 160), (480, 544))                                     # channels with count 0: 64 in a row, across two waves of the scan each


@functools.lru_cache(maxsize=None)
def _many_channels(n_chan):
    rng = _rng(8, n_chan)
    words = pool(_rng(8), 8)                                            # one pool for all channels and all cases
    chans = []
    for i in range(n_chan):
        cnt = 0 if any(a <= i < b for a, b in ZERO_RUNS) else int(rng.integers(0, 5))
        bp = [(q, words[rng.integers(8)], int(rng.integers(0, 175))) for q in range(4) if rng.random() < 0.6]
        if i == n_chan - 1 and n_chan > 1:                              # the last channel decodes for certain: its records land behind all the carries
            cnt, bp = 4, bp + [(0, words[rng.integers(8)], 50)]
        osd = [(q, words[rng.integers(8)], int(rng.integers(0, 175))) for q in range(4) if rng.random() < 0.5]
        chans.append(ft8_channel(rng, 3 * i + 1, 4, cnt, bp=bp, osd=osd, poison=words))
    return tuple(chans)


def ft8_channels():
    """1, 255, 256, 257 and 600 FT8 channels of four entries on a shared pool of 8 words: the scan's wave offsets and its carry add non-zero
    counts everywhere."""
    out = [_case(f"ft8_channels_{n}", 0, list(_many_channels(n))) for n in N_CHANNELS]
    for case in out[1:]:                                                # (one channel has neither a wave nor a run of 64 to fill)
        counts = answer(case)[1]
        assert all(any(counts[b:b + 64]) for b in range(0, len(counts), 64)) and any(not any(counts[b:b + 64]) for b in range(len(counts) - 63))
    return out


def truncation():
    """The 600-channel case and the crowded FT8 channel cut at max_out: 0, 1, around 256, around the total, and inside a channel."""
    out = []
    for name, chans in (("ft8_channels_600", list(_many_channels(600))), ("ft8_crowded", [_crowded_channel(False)])):
        recs, counts = answer(dict(ft4=0, channels=chans))
        total = len(recs)
        offs = np.concatenate([[0], np.cumsum(counts)])
        # between the two decodes of the last channel that has two; the single channel: anywhere
        edges = (0, 1, 255, 256, 257, total - 1, total, total + 8)
        inside = 100 if len(chans) == 1 else next(int(offs[i]) + 1 for i in range(len(counts) - 1, -1, -1) if counts[i] >= 2 and offs[i] + 1 not in edges)
        for mx in edges + (inside,):
            out.append(_case(f"{name}_max{mx}", 0, chans, max_out=mx))
    return out


FAMILIES = dict(ft8_distinct=ft8_distinct, ft8_crowded=ft8_crowded, ft8_one_word=ft8_one_word, ft8_rank_across_passes=ft8_rank_across_passes,
                ft8_keys=ft8_keys, ft4_crowded=ft4_crowded, ft4_small=ft4_small, ft8_channels=ft8_channels, truncation=truncation)


@functools.lru_cache(maxsize=None)
def family(name):
    return tuple(FAMILIES[name]())


@functools.lru_cache(maxsize=None)
def expected(name):
    """Per case of the family: (counts, offsets, out) the kernel must leave.  Cases that share their channels share the answer."""
    out, memo = [], {}
    for case in family(name):
        key = tuple(id(ch) for ch in case["channels"])
        if key not in memo:
            memo[key] = answer(case)
        out.append(blocks(case, *memo[key]))
    return tuple(out)


def all_cases():
    """[(family, index, case)] in the order of the case file."""
    return [(name, i, case) for name in FAMILIES for i, case in enumerate(family(name))]
