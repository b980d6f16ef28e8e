"""CPU: tests/shim_ft4_subtract_check.cpp -- cwslgpu::Context::subtractFt4, ft4Residual, ft4ResidualDevice, ft4SubtractFlat and the layouts of
cwslg_subtract_report and cwslg_ft4_sub_item -- is self-contained C++17 against the C ABI."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_ft4_subtract_check_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", os.path.join(ROOT, "tests", "shim_ft4_subtract_check.cpp")])
