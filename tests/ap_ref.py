"""Test helper: the numpy restatement of FT8 a-priori decoding (include/cwsl_gpu.h, "FT8 a-priori decoding": cwslg_ap_pattern, cwslg_ap_msg) --
per metric set the caller's patterns in order, the masked metrics replaced by +-A, the decode contract's loop on the result, the success rule and
the record with nharderr and dmin against the ORIGINAL metrics -- plus the setter's validation.  PARITY UNPINNED like the rest of the chain: this
is the repository's own statement; the GPU kernel (csrc/ap_kernels.hpp) and the host header (csrc/ap_host.hpp) are compared with it bit for bit.

The loop is written out here a second time (bp below keeps the whole codeword, which ldpc_ref.decode does not hand out); tests/test_ap_ref.py
holds the two texts together: an empty mask gives ldpc_ref.decode's record on the same metrics."""
import numpy as np

import ldpc_ref as R

F32 = np.float32
N, K, M, ROWMAX = R.N, R.K, R.M, R.ROWMAX
MAXPAT = 8
PATTERN_DTYPE = np.dtype([("mask", np.uint8, 12), ("value", np.uint8, 12)])
AP_MSG_DTYPE = np.dtype([("msg", R.MSG_DTYPE), ("dmin", np.float32)])
assert PATTERN_DTYPE.itemsize == 24 and AP_MSG_DTYPE.itemsize == 24


def make_patterns(pairs):
    """[(mask bits[<= 96], value bits[<= 96]), ...] as 0/1 sequences over codeword positions -> PATTERN_DTYPE array (MSB first, like bits[12])."""
    out = np.zeros(len(pairs), PATTERN_DTYPE)
    for i, (m, v) in enumerate(pairs):
        mm, vv = np.zeros(96, np.uint8), np.zeros(96, np.uint8)
        mm[:len(m)] = np.asarray(m, np.uint8)
        vv[:len(v)] = np.asarray(v, np.uint8)
        out["mask"][i], out["value"][i] = np.packbits(mm), np.packbits(vv)
    return out


def validate(patterns, n_pat=None, max_iter=30, min_nsync=7):
    """What cwslg_set_ft8_ap answers: 0, or the reason -- 1 n_pat outside 0..8, 2 a mask or value bit at position 91..95, 3 a value bit outside
    its mask (patterns in order, positions in order, the first finding; csrc/ap_host.hpp:ap_pack walks them the same way), 4 max_iter outside
    1..200 or min_nsync outside 0..22 (checked first)."""
    if not (1 <= max_iter <= 200) or not (0 <= min_nsync <= 22):
        return 4
    n_pat = len(patterns) if n_pat is None else n_pat
    if n_pat < 0 or n_pat > MAXPAT:
        return 1
    for p in range(n_pat):
        m, v = np.unpackbits(patterns["mask"][p]), np.unpackbits(patterns["value"][p])
        for t in range(96):
            if t >= 91 and (m[t] or v[t]):
                return 2
            if v[t] and not m[t]:
                return 3
    return 0


def pack_block(patterns):
    """The 192-byte block the kernel reads (csrc/ap_host.hpp: ApBlock): uint32[8][6], codeword bit t at bit t & 31 of word t >> 5; words 0..2 the
    mask, 3..5 the value."""
    w = np.zeros((MAXPAT, 6), np.uint32)
    for p in range(len(patterns)):
        for half, name in ((0, "mask"), (3, "value")):
            b = np.unpackbits(patterns[name][p])
            for t in range(96):
                if b[t]:
                    w[p, half + (t >> 5)] |= np.uint32(1 << (t & 31))
    return w


def bp(code, llr, max_iter):
    """The decode contract's loop (steps 1-8 of cwslg_ft8_msg) on llr float32[q, 174] -> (cw bool[q, 174], iters[q], nbad[q]) at exit.  All sets
    advance in lock step; a set that has left is frozen."""
    llr = np.ascontiguousarray(llr, dtype=F32).reshape(-1, N)
    Q = len(llr)
    cw_out, iters, nbad_out = np.zeros((Q, N), bool), np.zeros(Q, int), np.zeros(Q, int)
    live = np.arange(Q)
    v = np.zeros((Q, M * 8), F32)
    ncnt, nclast = np.zeros(Q, int), np.zeros(Q, int)
    rb = np.where(code.present, code.rowbit, 0)
    epos = (8 * np.arange(M).reshape(-1, 1) + np.arange(ROWMAX)).astype(np.int64)
    it = 0
    while live.size:
        L, vv = llr[live], v[live]
        z = ((L + vv[:, code.slot[:, 0]]) + vv[:, code.slot[:, 1]]) + vv[:, code.slot[:, 2]]
        assert z.dtype == F32
        cw = z > 0
        nbad = ((cw[:, rb] & code.present).sum(axis=2) & 1).sum(axis=1)
        done = (nbad == 0) | (it == max_iter)
        if it > 0:
            ncnt[live] = np.where(nbad - nclast[live] < 0, 0, ncnt[live] + 1)
            done |= (ncnt[live] >= 5) & (it >= 10) & (nbad > 15)
        d = live[done]
        cw_out[d], iters[d], nbad_out[d] = cw[done], it, nbad[done]
        nclast[live] = nbad
        keep = ~done
        live, z, vv = live[keep], z[keep], vv[keep]
        if not live.size:
            break
        t = R.T(F32(-0.5) * (z[:, rb] - vv[:, epos]))
        new = vv.copy()
        for e in range(ROWMAX):
            p = np.ones((live.size, M), F32)
            for f in range(ROWMAX):
                if f != e:
                    p = np.where(code.present[:, f], p * t[:, :, f], p)
            assert p.dtype == F32
            val = F32(2) * R.A(-p)
            rows = code.present[:, e]
            new[:, epos[rows, e]] = val[:, rows]
        v[live] = new
        it += 1
    return cw_out, iters, nbad_out


def distance(llr, cw):
    """OSD's d(c) (rule 7 of cwslg_osd_msg) of the word cw against the metrics llr: float32 adds of |llr[t]| over the t with (llr[t] > 0) != cw[t],
    ascending t, from +0."""
    a = np.abs(np.asarray(llr, F32))
    d = F32(0)
    for t in np.nonzero((np.asarray(llr, F32) > 0) != np.asarray(cw, bool))[0]:
        d = F32(d + a[t])
    return d


def decode(code, llr, patterns, max_iter, attempt=None, loop=bp):
    """llr float32[q, 174], patterns PATTERN_DTYPE[1..8] -> AP_MSG_DTYPE[q].  attempt bool[q] (None: all) is the caller's gate; a set with a
    metric that is not finite is not attempted either.  loop: the decode loop (a test may put a stub in its place to show a rule on its own)."""
    llr = np.ascontiguousarray(llr, dtype=F32).reshape(-1, N)
    Q = len(llr)
    assert validate(patterns, max_iter=max_iter) == 0 and len(patterns) >= 1
    out = np.zeros(Q, AP_MSG_DTYPE)
    msg = out["msg"]
    attempt = (np.ones(Q, bool) if attempt is None else np.asarray(attempt, bool)) & np.isfinite(llr).all(axis=1)
    msg["iters"][~attempt] = msg["nbad"][~attempt] = msg["nharderr"][~attempt] = -1
    msg["pad_"] = 0xff
    msg["nharderr"][attempt] = -1
    A = (F32(1.01) * np.abs(llr).max(axis=1)).astype(F32) if Q else np.zeros(0, F32)
    assert A.dtype == F32
    open_ = np.nonzero(attempt)[0]                                      # attempted, no success yet
    total = np.zeros(Q, int)
    for p in range(len(patterns)):
        if not open_.size:
            break
        mask = np.unpackbits(patterns["mask"][p])[:K].astype(bool)
        value = np.unpackbits(patterns["value"][p])[:K].astype(bool)
        lp = llr[open_].copy()
        forced = np.where(value[None, :], A[open_, None], -A[open_, None]).astype(F32)
        lp[:, :K] = np.where(mask[None, :], forced, lp[:, :K])
        cw, iters, nbad = loop(code, lp, max_iter)
        total[open_] += iters
        msg["iters"][open_] = total[open_]
        msg["nbad"][open_] = nbad
        ok = np.zeros(open_.size, bool)
        for j, q in enumerate(open_):
            ok[j] = (nbad[j] == 0 and R.crc14(cw[j][:77]) == R.crc_field(cw[j][:K]) and (cw[j][:K][mask] == value[mask]).all())
            if ok[j]:
                msg[q] = (R.pack_bits(cw[j]), iters[j], 0, int(((llr[q] > 0) != cw[j]).sum()), 1, p)
                out["dmin"][q] = distance(llr[q], cw[j])
        open_ = open_[~ok]
    return out


def fetch_gate(msg, osd, nsync, min_nsync):
    """cwslg_fetch_ft8_ap's attempt gate without rule 1 (decode() adds it): the decode record attempted without crc_ok; the OSD records not used
    (osd None) or without crc_ok; nsync >= min_nsync."""
    g = (msg["iters"] >= 0) & (msg["crc_ok"] == 0) & (np.asarray(nsync) >= min_nsync)
    if osd is not None:
        g &= osd["crc_ok"] == 0
    return g
