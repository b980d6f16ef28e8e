"""CPU: tests/shim_ft4_decode_reports_check.cpp -- cwslgpu::Context::fetchFt4DecodeReports, ft4Tones and the reuse of cwslg_decode_report -- is
self-contained C++17 against the C ABI; the two exports are declared by the header and listed by the binding."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_ft4_decode_reports_check_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", os.path.join(ROOT, "tests", "shim_ft4_decode_reports_check.cpp")])


def test_the_binding_lists_the_exports():
    from cwsl_digi_amd import api
    assert "cwslg_fetch_ft4_decode_reports" in api.ABI_SYMBOLS and "cwslg_ft4_tones" in api.ABI_SYMBOLS
    assert callable(api.Context.fetch_ft4_decode_reports) and callable(api.Context.ft4_tones)
    header = open(os.path.join(ROOT, "include", "cwsl_gpu.h")).read()
    assert "int cwslg_fetch_ft4_decode_reports(cwslg_ctx *ctx, uint64_t *start_epoch" in header and "int cwslg_ft4_tones(cwslg_ctx *ctx" in header
    assert "#define CWSLG_ABI_VERSION 5" in header
