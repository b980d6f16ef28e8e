"""CPU: the shim's FT4 a-priori wrappers compile against the C ABI, and apSetSplit (C++) equals api.ap_set_split (Python) on every value of the
`set` byte: set & 3 the metric set, set >> 2 the pattern."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "shim_ft4_ap_check.cpp")


def test_wrappers_compile():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", SRC])


def test_set_split_helpers_agree(tmp_path):
    from cwsl_digi_amd.api import ap_set_split
    exe = str(tmp_path / "shim_ft4_ap_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DSHIM_FT4_AP_CHECK_MAIN", SRC, "-o", exe])
    got = [tuple(int(x) for x in line.split()) for line in subprocess.run([exe], stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()]
    assert len(got) == 256
    s, p = ap_set_split(np.arange(256, dtype=np.uint8))
    assert got == [(v, int(s[v]), int(p[v])) for v in range(256)]
    assert all(ap_set_split(v) == (v & 3, v >> 2) for v in range(256))
    assert ap_set_split(2 | 7 << 2) == (2, 7)                           # the largest pair the call emits: set 2, pattern 7
