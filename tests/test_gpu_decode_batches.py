"""GPU: the stand-alone entry points of the two decode kernels (cwslg_ldpc_decode -> ldpc_decode_kernel, cwslg_osd_decode -> osd_decode_kernel) on
the large mixed batches of tests/decode_batch_cases.py: 1025 sets per code for belief propagation at max_iter 5, 30 and 200 (257 workgroups; every
exit, every branch of T and A, subnormal and huge metrics, exact zeros and ties, one infinite metric), 261 of them for OSD at orders 0, 1 and 2.
tests/test_decode_batch_inputs.py shows on the CPU what the batches hold.

Standard of comparison: every record BYTE-EQUAL to the numpy restatement (tests/ldpc_ref.py, tests/osd_ref.py), none tolerated.  The only sets
left out are belief propagation's NaN SETS (the contract expects finite metrics there): they must come back with 0 <= iters <= max_iter and must
not disturb the sets they share a workgroup with, which ARE compared.  OSD's NaN and inf sets are compared: they are not-attempted records.

Wall times: NOT YET RECORDED.  At the time of this commit the module had been collected and its inputs vetted on the CPU, but it had not run on an
MI355X; the first GPU run must record each test's wall time here (the yardstick is a few seconds each; the restatements' records are cached per
process: about 6 s for belief propagation at the three limits under both codes and about 12 s for OSD at the three orders, measured through the
CPU module).
"""
import numpy as np
import pytest

import decode_batch_cases as D
import ldpc_cases as C
import ldpc_ref as R
import osd_ref as O

pytestmark = pytest.mark.gpu


@pytest.fixture
def xctx():
    """A fresh context in the default (exact) arithmetic mode."""
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


def _same_msg(got, want, nan, max_iter):
    """Every record outside the NaN sets equals the restatement's; the NaN sets have left the loop in bounds."""
    assert got.dtype == want.dtype == R.MSG_DTYPE and got.shape == want.shape == nan.shape, (got.shape, want.shape)
    bad = [q for q in np.nonzero(~nan)[0] if got[q].tobytes() != want[q].tobytes()]
    assert not bad, (len(bad), bad[:5], [(got[q], want[q]) for q in bad[:3]])
    assert (got["iters"][nan] >= 0).all() and (got["iters"][nan] <= max_iter).all(), got[nan]
    return int((~nan).sum())


def _same_osd(got, want):
    assert got.dtype == want.dtype == O.OSD_DTYPE and got.shape == want.shape, (got.shape, want.shape)
    bad = [q for q in range(len(want)) if got[q].tobytes() != want[q].tobytes()]
    assert not bad, (len(bad), bad[:5], [(got[q], want[q]) for q in bad[:3]])


# ---- belief propagation ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", D.SEEDS)
@pytest.mark.parametrize("max_iter", D.MAX_ITERS)
def test_ldpc_batch_is_the_restatement(xctx, max_iter, seed):
    """1025 sets in one launch: all but the 24 NaN sets byte-equal, those in bounds, their workgroup neighbours among the compared."""
    b = D.batch(seed)
    xctx.set_ldpc_code(C.make_code(seed)["nm"])
    got = xctx.ldpc_decode(b["llr"], max_iter)
    assert _same_msg(got, D.ldpc_reference(seed, max_iter), b["nan"], max_iter) == D.NSETS - 24
    for q in np.nonzero(b["nan"])[0]:                                  # (said again where it matters: each NaN set has compared neighbours)
        assert not b["nan"][4 * (q // 4):4 * (q // 4) + 4].all()


@pytest.mark.parametrize("seed", D.SEEDS)
def test_ldpc_batch_twice_and_in_a_second_context(xctx, seed):
    """The same batch twice in one context and once in another: three times the same bytes, the NaN sets' records included."""
    import cwsl_digi_amd as P
    b = D.batch(seed)
    xctx.set_ldpc_code(C.make_code(seed)["nm"])
    first = xctx.ldpc_decode(b["llr"], 200)
    second = xctx.ldpc_decode(b["llr"], 200)
    with P.Context(0) as other:
        other.set_ldpc_code(C.make_code(seed)["nm"])
        third = other.ldpc_decode(b["llr"], 200)
    assert first.tobytes() == second.tobytes() == third.tobytes()
    _same_msg(first, D.ldpc_reference(seed, 200), b["nan"], 200)


@pytest.mark.parametrize("n", [1025, 1024, 1023])
def test_ldpc_batch_edges(xctx, n):
    """257 workgroups whose last holds one wave; 256 full ones; 255 and three waves, the input a slice of the same host array (not a fresh
    allocation): records 0..n-1 are the batch's."""
    seed = D.SEEDS[1]
    b = D.batch(seed)
    llr = b["llr"][:n]
    assert llr.ctypes.data == b["llr"].ctypes.data and llr.flags.c_contiguous and (n == D.NSETS or not llr.flags.owndata)
    xctx.set_ldpc_code(C.make_code(seed)["nm"])
    got = xctx.ldpc_decode(llr, 30)
    assert len(got) == n
    _same_msg(got, D.ldpc_reference(seed, 30)[:n], b["nan"][:n], 30)


# ---- OSD ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", D.SEEDS)
@pytest.mark.parametrize("order", D.ORDERS)
def test_osd_batch_is_the_restatement(xctx, order, seed):
    """261 sets in one launch (65 workgroups and one wave): every record byte-equal, the not-attempted ones (NaN, inf) included."""
    xctx.set_ldpc_code(C.make_code(seed)["nm"])
    llr = D.osd_sets(seed)
    got = xctx.osd_decode(llr, order)
    _same_osd(got, D.osd_reference(seed, order))
    na = ~np.isfinite(llr).all(axis=1)
    assert na.sum() == 24 and all(r.tobytes() == O.NOT_ATTEMPTED.tobytes() for r in got[na])
    if order == 2:
        assert xctx.osd_decode(llr, order).tobytes() == got.tobytes()  # the same call again: the same bytes


# ---- both kernels in one context ------------------------------------------------------------------------------------------------------------------
def test_both_kernels_in_one_context_and_a_second_code(xctx):
    """ldpc_decode, osd_decode, ldpc_decode again in one context: each gives what it gives alone (the restatement's records; the NaN sets' bytes
    repeat).  Then the other code is loaded and both run again, on that code's batch."""
    ctx = xctx
    a, b = D.SEEDS
    first_nan = None
    for seed in (a, b):
        bt = D.batch(seed)
        ctx.set_ldpc_code(C.make_code(seed)["nm"])
        m1 = ctx.ldpc_decode(bt["llr"], 30)
        o1 = ctx.osd_decode(D.osd_sets(seed), 1)
        m2 = ctx.ldpc_decode(bt["llr"], 30)
        _same_msg(m1, D.ldpc_reference(seed, 30), bt["nan"], 30)
        _same_osd(o1, D.osd_reference(seed, 1))
        assert m2.tobytes() == m1.tobytes()
        if first_nan is None:
            first_nan = m1[bt["nan"]].tobytes()
    # back to the first code: nothing of the second has stayed behind
    bt = D.batch(a)
    ctx.set_ldpc_code(C.make_code(a)["nm"])
    m3 = ctx.ldpc_decode(bt["llr"], 30)
    _same_msg(m3, D.ldpc_reference(a, 30), bt["nan"], 30)
    assert m3[bt["nan"]].tobytes() == first_nan
    _same_osd(ctx.osd_decode(D.osd_sets(a), 1), D.osd_reference(a, 1))
