"""CPU: tests/shim_decode_reports_check.cpp -- cwslgpu::Context::fetchDecodeReports, ft8Tones and the layout of cwslg_decode_report -- is
self-contained C++17 against the C ABI."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_decode_reports_check_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", os.path.join(ROOT, "tests", "shim_decode_reports_check.cpp")])
