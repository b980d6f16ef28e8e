"""Test helper: the numpy restatement of cwslg_osd_msg (include/cwsl_gpu.h, "FT8 OSD") -- ordered-statistics decoding, order 0, 1 or 2, of a
(174, 91) code whose parity-check table is data.  Integers throughout except the distance, float32 adds in ascending position.  PARITY UNPINNED:
this is the repository's own statement of OSD on the channel metrics, not upstream osd174_91; the GPU kernel (csrc/osd_kernels.hpp) and the host
header (csrc/ldpc_host.hpp: osd_host) are compared with it bit for bit.

The result does NOT depend on which generator of the code is fed in: step 3 asks whether a column is independent of the columns taken, which is a
property of the code (a change of basis multiplies every column by the same invertible matrix), and step 4's g_i are unique codewords.
tests/test_osd_ref.py shows it on two bases."""
import numpy as np

import ldpc_ref as R

F32 = np.float32
N, K, M = R.N, R.K, R.M
NPAIR = K * (K - 1) // 2
OSD_DTYPE = np.dtype([("bits", np.uint8, 12), ("dmin", np.float32), ("nharderr", np.int16), ("nskip", np.int16), ("crc_ok", np.uint8), ("how", np.uint8),
                      ("flip", np.uint8, 2)])
assert OSD_DTYPE.itemsize == 24
NOT_ATTEMPTED = np.zeros(1, OSD_DTYPE)
NOT_ATTEMPTED["nharderr"] = NOT_ATTEMPTED["nskip"] = -1
NOT_ATTEMPTED["how"] = 0xff
NOT_ATTEMPTED["flip"] = 0xff
PAIRS = np.array([(i, j) for i in range(K) for j in range(i + 1, K)])          # the tie rule's order: smaller i, then smaller j


def gf2_rank(A):
    A = np.array(A, np.uint8) % 2
    r = 0
    for c in range(A.shape[1]):
        rows = np.nonzero(A[r:, c])[0]
        if rows.size == 0:
            continue
        A[[r, r + rows[0]]] = A[[r + rows[0], r]]
        low = np.nonzero(A[:, c])[0]
        A[low[low != r]] ^= A[r]
        r += 1
        if r == A.shape[0]:
            break
    return r


def generator(H):
    """A basis of the null space of H (uint8[83, 174]) as uint8[174 - rank, 174]: row k carries the k-th free column (ascending) alone among the
    free columns (csrc/ldpc_host.hpp:ldpc_generator makes the same one).  -> (G, rank)."""
    A = np.array(H, np.uint8) % 2
    piv, r = [], 0
    for c in range(A.shape[1]):
        rows = np.nonzero(A[r:, c])[0]
        if rows.size == 0:
            continue
        A[[r, r + rows[0]]] = A[[r + rows[0], r]]
        low = np.nonzero(A[:, c])[0]
        A[low[low != r]] ^= A[r]
        piv.append(c)
        r += 1
        if r == A.shape[0]:
            break
    free = [c for c in range(A.shape[1]) if c not in set(piv)]
    G = np.zeros((len(free), A.shape[1]), np.uint8)
    for k, f in enumerate(free):
        G[k, f] = 1
        G[k, piv] = A[:r, f]
    return G, r


def pack_generator(G):
    """uint8[91, 174] -> the 2184-byte device block: 6 little-endian dwords per row, bit t of the row at dword t >> 5, bit t & 31."""
    b = np.zeros((K, 192), np.uint8)
    b[:, :N] = G
    return np.packbits(b, axis=1, bitorder="little").tobytes()


def reliability_order(a):
    """Positions by descending a, ties by ascending index."""
    return np.array(sorted(range(N), key=lambda t: (-float(a[t]), t)))


def most_reliable_basis(G, order):
    """Steps 3 and 4.  -> (p int[91], nskip, g uint8[91, 174])."""
    G = np.array(G, np.uint8) % 2
    taken = np.zeros((0, K), np.uint8)               # the columns taken, reduced against each other, one per row, with their leading index
    lead = []
    p, walked = [], 0
    for t in order:
        walked += 1
        col = G[:, t].copy()
        for row, l in zip(taken, lead):              # reduce the column by the echelon set: independent iff something is left
            if col[l]:
                col ^= row
        if not col.any():
            continue
        lead.append(int(np.nonzero(col)[0][0]))
        taken = np.vstack([taken, col])
        p.append(int(t))
        if len(p) == K:
            break
    assert len(p) == K, "the generator's rank is below 91"
    B = G[:, p]                                      # 91 x 91, invertible: g = B^-1 G has g[:, p] = I
    A = np.concatenate([B, G], axis=1)
    for c in range(K):
        rows = np.nonzero(A[c:, c])[0]
        A[[c, c + rows[0]]] = A[[c + rows[0], c]]
        low = np.nonzero(A[:, c])[0]
        A[low[low != c]] ^= A[c]
    g = A[:, K:]
    assert np.array_equal(g[:, p], np.eye(K, dtype=np.uint8))
    return np.array(p), walked - K, g


def distances(E, a):
    """E uint8[n, 174] error patterns -> float32[n]: (((+0 + m_0 a[0]) + m_1 a[1]) + ...), one float32 add per position in ascending order."""
    d = np.zeros(len(E), F32)
    zero = F32(0)
    for t in range(N):
        d = d + np.where(E[:, t] != 0, a[t], zero).astype(F32)
        assert d.dtype == F32
    return d


def candidates(g, c0, order):
    """-> (words uint8[n, 174], flips [(how, i, j)]) in the tie rule's order."""
    words, flips = [c0[None, :]], [(0, 0xff, 0xff)]
    if order >= 1:
        words.append(c0[None, :] ^ g)
        flips += [(1, i, 0xff) for i in range(K)]
    if order >= 2:
        words.append(c0[None, :] ^ g[PAIRS[:, 0]] ^ g[PAIRS[:, 1]])
        flips += [(2, int(i), int(j)) for i, j in PAIRS]
    return np.concatenate(words), flips


def decode_one(G, llr, order):
    """One set of metrics -> a record (OSD_DTYPE scalar array of length 1)."""
    llr = np.asarray(llr, F32)
    a = np.abs(llr)
    if not np.isfinite(a).all():
        return NOT_ATTEMPTED.copy()
    hard = (llr > 0).astype(np.uint8)
    p, nskip, g = most_reliable_basis(G, reliability_order(a))
    c0 = (hard[p].astype(int) @ g.astype(int) % 2).astype(np.uint8)
    words, flips = candidates(g, c0, order)
    d = distances(words ^ hard[None, :], a)
    w = int(np.argmin(d))                            # the first of the smallest: the candidates are in the tie rule's order
    cw = words[w]
    how, i, j = flips[w]
    out = np.zeros(1, OSD_DTYPE)
    out[0] = (R.pack_bits(cw), d[w], int((cw != hard).sum()), nskip, int(R.crc14(cw[:77]) == R.crc_field(cw[:K])), how, (i, j))
    return out


def decode(G, llr, order, attempt=None):
    """llr float32[q, 174] -> records OSD_DTYPE[q]; attempt bool[q] (None: all)."""
    llr = np.ascontiguousarray(llr, dtype=F32).reshape(-1, N)
    attempt = np.ones(len(llr), bool) if attempt is None else np.asarray(attempt, bool)
    out = np.zeros(len(llr), OSD_DTYPE)
    for q in range(len(llr)):
        out[q] = (decode_one(G, llr[q], order) if attempt[q] else NOT_ATTEMPTED)[0]
    return out


def chain_records(G, llr, order, nsync, msg, min_nsync):
    """decode() with the chain's gates: candidate q is attempted iff its decode record was attempted (iters >= 0) and has crc_ok == 0 and its
    soft-bit record has nsync >= min_nsync."""
    return decode(G, llr, order, (msg["iters"] >= 0) & (msg["crc_ok"] == 0) & (np.asarray(nsync) >= min_nsync))
