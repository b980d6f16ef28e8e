"""CPU: tests/shim_decodes_check.cpp -- cwslgpu::Context::fetchDecodes and the layout of cwslg_decode -- is self-contained C++17 against the C ABI."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shim_decodes_check_compiles():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", os.path.join(ROOT, "tests", "shim_decodes_check.cpp")])
