"""GPU: the a-priori decode (ap_decode_kernel) through cwslg_ap_decode against the numpy restatement (tests/ap_ref.py), BYTE FOR BYTE -- no tolerance anywhere: the mixed
batch of tests/ap_cases.py at every size that changes the grid, under 1, 2 and 8 patterns; every hand-made case of tests/test_ap_ref.py; nothing
written beyond record n; a second code and other patterns between calls; the argument errors."""
import numpy as np
import pytest

import ap_cases as C
import ap_ref as AP
import ldpc_cases as LC

pytestmark = pytest.mark.gpu
ARG = -6


@pytest.fixture
def xctx():
    import cwsl_digi_amd as P
    c = P.Context(0)
    yield c
    c.close()


def _same(got, want):
    assert got.dtype == want.dtype == AP.AP_MSG_DTYPE and got.shape == want.shape, (got.shape, want.shape)
    bad = [q for q in range(len(want)) if got[q].tobytes() != want[q].tobytes()]
    assert not bad, (bad[:5], [(got[q], want[q]) for q in bad[:3]])


@pytest.mark.parametrize("n_pat", C.BATCH_NPAT)
@pytest.mark.parametrize("n", C.BATCH_SIZES)
def test_batch_is_the_restatement(xctx, n, n_pat):
    """Empty, one wave, a partial and a full workgroup, the step into the next, 63 / 64 / 65 and 257 sets (65 workgroups)."""
    xctx.set_ldpc_code(LC.make_code(C.SEED)["nm"])
    xctx.set_ft8_ap(C.patterns(n_pat), C.MAX_ITER, 7)
    got = xctx.ap_decode(C.batch()[0][:n])
    _same(got, C.batch_reference(n_pat)[:n])
    if n == C.BATCH_N:
        assert got["msg"]["crc_ok"].sum() >= 20 and (got["msg"]["iters"] == -1).sum() == 2      # finds, and the two sets that are not finite


@pytest.mark.parametrize("name", sorted(C.rule_cases()))
def test_rule_cases_are_the_restatement(xctx, name):
    pat, x, _ = C.rule_cases()[name]
    xctx.set_ldpc_code(LC.make_code(C.SEED)["nm"])
    xctx.set_ft8_ap(pat, C.MAX_ITER, 7)
    _same(xctx.ap_decode(x[None]), AP.decode(LC.make_code(C.SEED)["code"], x[None], pat, C.MAX_ITER))


def test_nothing_is_written_beyond_record_n(xctx):
    xctx.set_ldpc_code(LC.make_code(C.SEED)["nm"])
    xctx.set_ft8_ap(C.patterns(2), C.MAX_ITER, 7)
    n = 5
    llr = np.ascontiguousarray(C.batch()[0][:n])
    buf = np.full((n + 3) * 24, 0xAB, np.uint8)
    xctx._chk(xctx.L.cwslg_ap_decode(xctx.h, llr.ctypes.data, n, buf.ctypes.data))
    assert buf[:n * 24].tobytes() == C.batch_reference(2)[:n].tobytes() and (buf[n * 24:] == 0xAB).all()


def test_a_second_code_and_other_patterns_between_calls(xctx):
    a, b = LC.SEEDS
    llr = C.batch()[0][:65]
    xctx.set_ldpc_code(LC.make_code(a)["nm"])
    xctx.set_ft8_ap(C.patterns(2), C.MAX_ITER, 7)
    first = xctx.ap_decode(llr)
    _same(first, C.batch_reference(2)[:65])
    xctx.set_ldpc_code(LC.make_code(b)["nm"])                           # the first code's metrics under the second code
    second = xctx.ap_decode(llr)
    _same(second, AP.decode(LC.make_code(b)["code"], llr, C.patterns(2), C.MAX_ITER))
    assert first.tobytes() != second.tobytes()
    xctx.set_ldpc_code(LC.make_code(a)["nm"])
    xctx.set_ft8_ap(C.patterns(8), C.MAX_ITER, 7)                        # patterns replaced
    third = xctx.ap_decode(llr)
    _same(third, C.batch_reference(8)[:65])
    assert third.tobytes() != first.tobytes()
    xctx.set_ft8_ap(C.patterns(8)[::-1].copy(), 5, 0)                    # another order, another max_iter
    _same(xctx.ap_decode(llr), AP.decode(LC.make_code(a)["code"], llr, C.patterns(8)[::-1], 5))
    xctx.set_ft8_ap(C.patterns(2), C.MAX_ITER, 7)
    _same(xctx.ap_decode(llr), first)


def test_argument_errors(xctx):
    from cwsl_digi_amd.api import CwslGpuError

    def raises(fn, *a):
        with pytest.raises(CwslGpuError) as e:
            fn(*a)
        assert e.value.status == ARG, e.value

    llr = C.batch()[0][:3]
    ok = C.patterns(2)
    xctx.set_ft8_ap(ok, 30, 7)                                           # the setter needs no code
    raises(xctx.ap_decode, llr)                                         # no code loaded
    xctx.set_ldpc_code(LC.make_code(C.SEED)["nm"])
    want = xctx.ap_decode(llr)
    _same(want, C.batch_reference(2)[:3])
    assert len(xctx.ap_decode(llr[:0])) == 0                            # n = 0 is legal
    bad = C.patterns(8)
    bad["mask"][2][11] |= 0x10                                           # position 91
    raises(xctx.set_ft8_ap, bad, 30, 7)
    bad = C.patterns(8)
    bad["value"][5][4] |= 0x10                                           # a value bit outside its (empty) mask
    raises(xctx.set_ft8_ap, bad, 30, 7)
    raises(xctx.set_ft8_ap, np.zeros(9, AP.PATTERN_DTYPE), 30, 7)
    for it, ns in ((0, 7), (201, 7), (30, -1), (30, 23)):
        raises(xctx.set_ft8_ap, ok, it, ns)
    _same(xctx.ap_decode(llr), want)                                    # a rejected set leaves the patterns in force
    xctx.set_ft8_ap(ok[:0], 30, 7)                                       # n_pat = 0 clears them
    raises(xctx.ap_decode, llr)
    assert xctx.L.cwslg_ap_decode(None, llr.ctypes.data, 3, want.ctypes.data) == ARG
    assert xctx.L.cwslg_set_ft8_ap(None, ok.ctypes.data, 2, 30, 7) == ARG
