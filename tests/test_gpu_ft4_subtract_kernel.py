"""GPU: the FT4 subtractor's two kernels through cwslg_ft4_subtract_flat (include/cwsl_gpu.h, "FT4 signal subtraction"; modules/ft4sub.hip), byte for
byte against the numpy restatement (tests/ft4_subtract_ref.py) on tests/ft4_subtract_cases.py's frames; the roster of the module's code object
 and its freedom from scratch memory.
tests/ft4_subtract_edge_cases.py adds the inputs whose window starts have every remainder w0 mod 4, items at the limits of dt_s and freq_hz, and a
table of offsets with runs of equal entries (tests/test_subtract_edge_inputs.py: what each contains, on the CPU).
Times of the flat-call tests on one MI355X, the restatement on the host included (it is most of each): zero_one_four 0.10 s; offgrid 0.12, limits 0.13, crowded 0.48, reversed 0.42 (before its fits were shared with crowded's), trailing 0.02 s.  crowded is 27 fits of the restatement,
about 0.04 s each there, which is what it takes to put 24 records on one walk of the apply kernel."""
import os
import re

import numpy as np
import pytest

import ft4_subtract_cases as SC
import ft4_subtract_edge_cases as EC
import ft4_subtract_ref as S
import ldpc_cases as LC
import report_kernel_cases as K

ERR_ARG = -6

# Every kernel of cwslgpu_ft4sub.hsaco, by name, with its job.  The library's own roster (tests/test_abi_and_host.py) and the FT8 module's
# (tests/test_gpu_ft8_subtract_kernel.py) do not see this code object: a kernel added to it shows up HERE.
MODULE_ROSTER = {
    "ft4_sub_fit_kernel",        # one workgroup per emitted decode: refined frequency and start, amplitude track, report, the apply's record
    "ft4_sub_apply_kernel",      # one workgroup per (1024-sample tile, channel): frame minus the fitted waveforms, in emission order
}


def _module_path():
    from cwsl_digi_amd import build as B
    B.build()                                   # (a no-op when the libraries and the module are current)
    return B.FT4SUB_MODULE


def test_module_roster_and_no_scratch():
    """(no GPU needed: the code object is read as a file)  The kernel descriptors <name>.kd are the roster; the metadata note of every kernel
    says .private_segment_fixed_size: 0 -- no scratch."""
    data = open(_module_path(), "rb").read()
    names = set(m.decode() for m in re.findall(rb"([A-Za-z_][A-Za-z0-9_]*)\.kd", data))
    assert names == MODULE_ROSTER, sorted(names ^ MODULE_ROSTER)
    # the msgpack metadata: the key, then a positive fixint (0x00..0x7f) or a wider unsigned
    sizes = re.findall(rb"\.private_segment_fixed_size(.)", data, re.S)
    assert len(sizes) == len(MODULE_ROSTER) and all(s == b"\x00" for s in sizes), sizes
    # and neither the library nor the FT8 subtractor's module carries one of them (each roster is one kernel per job of ITS code object)
    from cwsl_digi_amd import build as B
    lib, ft8 = open(B.LIB, "rb").read(), open(B.FT8SUB_MODULE, "rb").read()
    # (the library holds the two names as the strings its loader looks up, never as kernels: no descriptor; the FT8 module holds neither name)
    assert not any(n.encode() + b".kd" in lib or n.encode() in ft8 for n in MODULE_ROSTER)


@pytest.fixture(scope="module")
def fctx():
    import cwsl_digi_amd as P
    c = P.Context(0)
    c.set_ldpc_code(LC.make_code(SC.SEED)["nm"])
    yield c
    c.close()


def _compare(got_sub, got_res, name, cases=SC):
    want_sub, want_res = cases.kernel_reference(name)
    assert got_sub.dtype.itemsize == S.SUB_DTYPE.itemsize and len(got_sub) == len(want_sub)
    bad = [i for i in range(len(want_sub)) if got_sub[i].tobytes() != want_sub[i].tobytes()]
    assert not bad, (bad, got_sub[bad[:3]], want_sub[bad[:3]])
    diff = np.flatnonzero(got_res.view(np.uint32).reshape(-1) != want_res.view(np.uint32).reshape(-1))
    assert diff.size == 0, (diff.size, diff[:5], got_res.reshape(-1)[diff[:5]], want_res.reshape(-1)[diff[:5]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one", "zero_one_four", "edges", "silence", "no_items"])
def test_flat_call_against_the_restatement(fctx, name):
    audio, items = SC.kernel_cases()[name]
    sub, res = fctx.ft4_subtract_flat(audio, items)
    _compare(sub, res, name)
    want_sub, want_res = SC.kernel_reference(name)
    if name == "silence":
        assert not res.view(np.uint32).any() and np.isfinite([float(sub[0][f]) for f in ("f_hz", "dt_s", "p_removed", "p_before", "p_after")]).all()
        assert sub["p_removed"][0] == 0
    if name == "no_items":
        assert res.tobytes() == audio.tobytes()
    if name == "zero_one_four":
        assert res[0].tobytes() == audio[0].tobytes()                   # the frame without an item: its own bits
        # (the frames do contain what the items name: the fits take energy out where a transmission is; item 2 is the weak one a strong
        # neighbour one tone spacing away overlaps: no joint fit)
        strong = [0, 1, 3, 4]
        assert (want_sub["p_removed"][strong] > 0.5 * want_sub["p_before"][strong]).all()
    if name == "edges":
        # one starts 1440 samples before sample 0, the other ends 1152 samples past 72576 (give or take the 54 samples of the time search)
        assert (want_sub["n_inside"] < S.NW).all() and (want_sub["n_inside"] > S.NW - 1500).all()
        assert want_sub["dt_s"][0] < -0.5 and want_sub["dt_s"][1] > 0.69


@pytest.mark.gpu
@pytest.mark.parametrize("name", EC.NAMES)
def test_flat_call_on_the_edge_cases(fctx, name):
    """tests/ft4_subtract_edge_cases.py (what each case contains: tests/test_subtract_edge_inputs.py): window starts with every remainder
    w0 mod 4, items at the limits of dt_s and freq_hz, 8 frames with items on three of them and 24 on one, those 24 in reverse order, and two
    trailing frames without an item"""
    audio, items = EC.kernel_cases()[name]
    sub, res = fctx.ft4_subtract_flat(audio, items)
    _compare(sub, res, name, EC)
    if name == "limits":
        assert np.isfinite([[float(sub[i][f]) for f in ("f_hz", "dt_s", "p_removed", "p_before", "p_after")] for i in range(len(sub))]).all()
        assert np.isfinite(res).all()
        for i in (0, 1):                                                # dt_s = +30, -30: wholly outside the frame
            assert abs(float(items["dt_s"][i])) == 30.0 and sub["n_inside"][i] == 0
            assert all(sub[f][i].tobytes() == np.float32(0).tobytes() for f in ("p_removed", "p_before", "p_after"))
    if name == "crowded":
        for f in (1, 2, 4, 5, 6):                                       # the frames without an item: their own bits
            assert res[f].tobytes() == audio[f].tobytes()
    if name == "trailing":
        assert res[1:].tobytes() == audio[1:].tobytes()


@pytest.mark.gpu
def test_flat_call_twice_and_without_residual(fctx):
    audio, items = SC.kernel_cases()["zero_one_four"]
    a = fctx.ft4_subtract_flat(audio, items)
    b = fctx.ft4_subtract_flat(audio, items)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    c = fctx.ft4_subtract_flat(audio, items, want_residual=False)
    assert c[1] is None and c[0].tobytes() == a[0].tobytes()


@pytest.mark.gpu
def test_flat_call_errors(fctx):
    import cwsl_digi_amd as P
    audio, items = SC.kernel_cases()["zero_one_four"]
    for bad in (items[::-1].copy(),):                                   # descending frames
        with pytest.raises(P.CwslGpuError) as e:
            fctx.ft4_subtract_flat(audio, bad)
        assert e.value.status == ERR_ARG
    for field, value in (("frame", 3), ("freq_hz", -1.0), ("freq_hz", np.nan), ("dt_s", 31.0), ("dt_s", np.inf)):
        it = items[-1:].copy()
        it[field] = value
        with pytest.raises(P.CwslGpuError) as e:
            fctx.ft4_subtract_flat(audio, it)
        assert e.value.status == ERR_ARG, field
    # a table without systematic form: no re-encoder, no subtraction; without a table neither
    with P.Context(0) as c:
        with pytest.raises(P.CwslGpuError) as e:
            c.ft4_subtract_flat(audio, items)
        assert e.value.status == ERR_ARG and "cwslg_set_ldpc_code" in str(e.value)
        c.set_ldpc_code(K.singular_table(SC.SEED))
        with pytest.raises(P.CwslGpuError) as e:
            c.ft4_subtract_flat(audio, items)
        assert e.value.status == ERR_ARG and "systematic" in str(e.value)


@pytest.mark.gpu
def test_missing_module_names_the_file(tmp_path):
    """A library loaded from a directory without the code object: CWSLG_ERR_ARG with a text that names the file it looked for.  (A copy of the
    library in an empty directory, driven in a fresh process: the module is found beside the library, by dladdr.)"""
    import shutil
    import subprocess
    import sys
    from cwsl_digi_amd import build as B
    lib = tmp_path / "libcwslgpu.so"
    shutil.copy(B.LIB, lib)
    code = r"""
import ctypes as C, sys
L = C.CDLL(sys.argv[1])
L.cwslg_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
L.cwslg_last_error.restype = C.c_char_p
L.cwslg_last_error.argtypes = [C.c_void_p]
h = C.c_void_p()
assert L.cwslg_create(C.byref(h), 0) == 0
nm = open(sys.argv[2], "rb").read()
L.cwslg_set_ldpc_code.argtypes = [C.c_void_p, C.c_char_p]
assert L.cwslg_set_ldpc_code(h, nm) == 0
audio = (C.c_float * 72576)()
L.cwslg_ft4_subtract_flat.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
rc = L.cwslg_ft4_subtract_flat(h, audio, 1, None, 0, None, None)
print(rc, L.cwslg_last_error(h).decode())
L.cwslg_destroy.argtypes = [C.c_void_p]
L.cwslg_destroy(h)
"""
    nm = tmp_path / "nm.bin"
    nm.write_bytes(np.ascontiguousarray(LC.make_code(SC.SEED)["nm"], np.uint8).tobytes())
    out = subprocess.run([sys.executable, "-c", code, str(lib), str(nm)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rc, text = out.stdout.strip().split(" ", 1)
    assert int(rc) == ERR_ARG and str(tmp_path / "cwslgpu_ft4sub.hsaco") in text, out.stdout
