"""Test helper: the numpy restatement of cwslg_ft8_msg (include/cwsl_gpu.h, "FT8 decode") -- flooding sum-product decoding of a (174, 91) code
whose parity-check table is data, float32 throughout, every product chain written out in the stated order -- plus the table validation, the
derived tables and the CRC-14.  PARITY UNPINNED like the rest of the sync stage: this is the repository's own statement, structured like upstream
bpdecode174_91; the GPU kernel (csrc/ldpc_kernels.hpp) and the host header (csrc/ldpc_host.hpp) are compared with it bit for bit."""
import numpy as np

F32 = np.float32
N, K, M, ROWMAX = 174, 91, 83, 7
MSG_DTYPE = np.dtype([("bits", np.uint8, 12), ("iters", np.int16), ("nbad", np.int16), ("nharderr", np.int16), ("crc_ok", np.uint8), ("pad_", np.uint8)])
assert MSG_DTYPE.itemsize == 20


def validate(nm):
    """0 for a good table, else the reason: 1 a position above 174, 2 a zero that is not the last entry of its row (a row lighter than 6
    included), 3 a position twice in a row, 4 a position that does not occur exactly three times.  Rows are read in order, entries in order, and
    the first finding is returned (csrc/ldpc_host.hpp:ldpc_derive walks the table the same way)."""
    nm = np.asarray(nm).reshape(M, ROWMAX)
    count = np.zeros(N, int)
    for m in range(M):
        for e in range(ROWMAX):
            v = int(nm[m, e])
            if v > N:
                return 1
            if v == 0:
                if e != ROWMAX - 1:
                    return 2
                continue
            if v in [int(x) for x in nm[m, :e]]:
                return 3
            if count[v - 1] >= 3:
                return 4
            count[v - 1] += 1
    return 0 if (count == 3).all() else 4


class Code:
    """The tables derived from nm[83][7]: rowbit[m, e] (0-based bit, -1 absent), weight[m], and per bit its three (row, entry) in ascending row
    order as slot[n, k] = 8 m + e (the kernel's message position)."""

    def __init__(self, nm):
        nm = np.asarray(nm, dtype=np.int64).reshape(M, ROWMAX)
        assert validate(nm) == 0
        self.nm = nm.astype(np.uint8)
        self.rowbit = nm - 1
        self.present = nm > 0
        self.weight = self.present.sum(axis=1)
        self.slot = np.zeros((N, 3), np.int64)
        self.kslot = np.full((M, ROWMAX), -1, np.int64)                   # the slot of row m in its bit: k with c(n, k) = m
        fill = np.zeros(N, int)
        for m in range(M):
            for e in range(ROWMAX):
                if self.present[m, e]:
                    n = self.rowbit[m, e]
                    self.slot[n, fill[n]] = 8 * m + e
                    self.kslot[m, e] = fill[n]
                    fill[n] += 1
        self.H = np.zeros((M, N), np.uint8)
        for m in range(M):
            self.H[m, self.rowbit[m, self.present[m]]] = 1


def T(x):
    x = np.asarray(x, F32)
    a = np.abs(x)
    with np.errstate(over="ignore", invalid="ignore"):
        x2 = a * a
        num = a * (F32(945) + x2 * (F32(105) + x2))
        den = F32(945) + x2 * (F32(420) + x2 * F32(15))
        r = np.minimum(num / den, F32(1))
    r = np.where(a >= F32(4.97), F32(1), r).astype(F32)
    return np.copysign(r, x)


def A(y):
    y = np.asarray(y, F32)
    z = np.abs(y)
    r = np.where(z <= F32(0.664), z / F32(0.83),
                 np.where(z <= F32(0.9217), (z - F32(0.4064)) / F32(0.322),
                          np.where(z <= F32(0.9951), (z - F32(0.8378)) / F32(0.0524),
                                   np.where(z <= F32(0.9998), (z - F32(0.9914)) / F32(0.0012), F32(7))))).astype(F32)
    return np.copysign(r, y)


def crc14(bits77):
    """Remainder (14 bits, as an int) of the 77 bits + 5 zero bits + 14 augmenting zero bits by 0x2757 with x^14 implicit."""
    rem = 0
    for i in range(77 + 5 + 14):
        rem = (rem << 1) | (int(bits77[i]) if i < 77 else 0)
        if rem & 0x4000:
            rem ^= 0x6757
    return rem


def crc_field(bits91):
    v = 0
    for i in range(14):
        v = (v << 1) | int(bits91[77 + i])
    return v


def pack_bits(cw):
    """Codeword bits 0..90 -> 12 bytes, MSB first, the last 5 bits 0."""
    b = np.zeros(96, np.uint8)
    b[:K] = np.asarray(cw[:K], np.uint8)
    return np.packbits(b)


def unpack_bits(bits12):
    return np.unpackbits(np.asarray(bits12, np.uint8))[:K]


def decode(code, llr, max_iter, attempt=None):
    """llr float32[q, 174] -> records MSG_DTYPE[q].  attempt bool[q] (None: all): a record that is not attempted has iters = nbad = nharderr = -1,
    zero bits and crc_ok = 0.  All attempted sets advance in lock step; a set that has left is frozen."""
    llr = np.ascontiguousarray(llr, dtype=F32).reshape(-1, N)
    Q = len(llr)
    out = np.zeros(Q, MSG_DTYPE)
    attempt = np.ones(Q, bool) if attempt is None else np.asarray(attempt, bool)
    out["iters"][~attempt] = out["nbad"][~attempt] = out["nharderr"][~attempt] = -1
    live = np.nonzero(attempt)[0]                                      # indices still iterating
    v = np.zeros((Q, M * 8), F32)                                      # message of edge (m, e) at 8 m + e
    ncnt, nclast = np.zeros(Q, int), np.zeros(Q, int)
    rb = np.where(code.present, code.rowbit, 0)
    epos = (8 * np.arange(M).reshape(-1, 1) + np.arange(ROWMAX)).astype(np.int64)      # [83, 7]
    it = 0
    while live.size:
        L = llr[live]
        vv = v[live]
        z = ((L + vv[:, code.slot[:, 0]]) + vv[:, code.slot[:, 1]]) + vv[:, code.slot[:, 2]]
        assert z.dtype == F32
        cw = z > 0
        par = (cw[:, rb] & code.present).sum(axis=2) & 1               # [q, 83]
        nbad = par.sum(axis=1)
        done = (nbad == 0) | (it == max_iter)
        if it > 0:
            nd = nbad - nclast[live]
            ncnt[live] = np.where(nd < 0, 0, ncnt[live] + 1)
            done |= (ncnt[live] >= 5) & (it >= 10) & (nbad > 15)
        for j in np.nonzero(done)[0]:
            q = live[j]
            ok = nbad[j] == 0 and crc14(cw[j][:77]) == crc_field(cw[j][:K])
            out[q] = (pack_bits(cw[j]), it, nbad[j], int(((L[j] > 0) != cw[j]).sum()), int(ok), 0)
        keep = ~done
        nclast[live] = nbad
        live, z, vv = live[keep], z[keep], vv[keep]
        if not live.size:
            break
        t = T(F32(-0.5) * (z[:, rb] - vv[:, epos]))                    # [q, 83, 7]; absent entries are never used
        new = vv.copy()
        for e in range(ROWMAX):
            p = np.ones((live.size, M), F32)
            for f in range(ROWMAX):
                if f != e:
                    p = np.where(code.present[:, f], p * t[:, :, f], p)
            assert p.dtype == F32
            val = F32(2) * A(-p)
            rows = code.present[:, e]
            new[:, epos[rows, e]] = val[:, rows]
        v[live] = new
        it += 1
    return out


def hard_records(code, llr, max_iter, nsync, sigma, min_nsync):
    """decode() with the chain's filter: a candidate whose nsync < min_nsync or whose sigma == 0 is not attempted."""
    return decode(code, llr, max_iter, (np.asarray(nsync) >= min_nsync) & (np.asarray(sigma) != 0))
