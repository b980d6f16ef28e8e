"""GPU: decode_report_kernel (csrc/harvest_kernels.hpp) alone, on planes, lists and records a test wrote -- wave
positions in the workgroup and the last partial workgroup, the plane's edges, row pitches 32 and 992, a plane of equal values, one huge among 78
tiny terms, the XOR reduction over both row halves of the encoder, 1, 2 and 257 channels with empty ones first, last and in a row, a limit below
and above the total.  tests/report_kernel_check.hip drives the kernel through report_launch, the launch of cwslg_fetch_decode_reports, once for
all cases of tests/report_kernel_cases.py in one child process; every comparison is byte for byte against tests/decode_reports_ref.py, and what
lies past the last report must still be 0xAB."""
import subprocess

import numpy as np
import pytest

import report_kernel_cases as K

pytestmark = pytest.mark.gpu
RUN_TIMEOUT_S = 120


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("report_kernel")
    exe = K.build_check_program(tmp)
    cs = K.cases()
    fin, fout = str(tmp / "cases.bin"), str(tmp / "results.bin")
    K.write_cases(fin, cs)
    try:
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=RUN_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        pytest.fail(f"report_kernel_check did not finish within {RUN_TIMEOUT_S} s")
    if p.returncode != 0:
        pytest.fail(f"report_kernel_check exit {p.returncode}: {p.stdout[-500:]} {p.stderr[-2000:]}")
    return dict(zip((c["name"] for c in cs), K.read_results(fout, cs)))


@pytest.mark.parametrize("name", [c["name"] for c in K.cases()])
def test_case(results, name):
    case = next(c for c in K.cases() if c["name"] == name)
    diff = K.first_difference(case, results[name], K.answer(case))
    assert not diff, diff


def test_guards_untouched(results):
    for case in K.cases():
        n = min(case["n_total"], case["lim"])
        assert (results[case["name"]][K.REP_WORDS * n:] == K.AB).all(), case["name"]
