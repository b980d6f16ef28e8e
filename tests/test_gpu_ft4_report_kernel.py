"""GPU: ft4_report_kernel (csrc/ft4soft_kernels.hpp) alone, on frame spectra, sync records and decode records a test
wrote -- 1, 2, 3 and 5 decodes, 600 candidates whose entry -> slot prefix crosses the passes of 256 and ends in the last slot, f1_hz at both ends
of the band and ibest at both extremes, a carrier halfway between two tones, the zero spectrum (every first maximum a tie), one huge term among
small ones on the lanes where the sum's pairing changes, the XOR reduction over both row halves of the encoder, 1, 2 and 257 channels with empty
ones first, last and 40 in a row, a limit below and above the total.  tests/ft4_report_kernel_check.hip drives the kernel through
ft4_report_launch, the launch of cwslg_fetch_ft4_decode_reports, once for all cases of tests/ft4_report_kernel_cases.py in one child process;
every comparison is byte for byte against tests/ft4_decode_reports_ref.py (xsig / xnoise: or NaN on both sides), and what lies past the last
report must still be 0xAB."""
import subprocess

import numpy as np
import pytest

import ft4_report_kernel_cases as K

pytestmark = pytest.mark.gpu
RUN_TIMEOUT_S = 120


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ft4_report_kernel")
    exe = K.build_check_program(tmp)
    cs = K.cases()
    fin, fout = str(tmp / "cases.bin"), str(tmp / "results.bin")
    K.write_cases(fin, cs)
    try:
        p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=RUN_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        pytest.fail(f"ft4_report_kernel_check did not finish within {RUN_TIMEOUT_S} s")
    if p.returncode != 0:
        pytest.fail(f"ft4_report_kernel_check exit {p.returncode}: {p.stdout[-500:]} {p.stderr[-2000:]}")
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
