"""CPU: csrc/record_kinds.hpp -- the kind table and the one epoch rule behind every record fetch, cwslg_fetch_slot and sync_launch's stamps --
against the conditions written out longhand in tests/record_kinds_check.cpp.  The check is a stand-alone program (its own main, no Python
extension, no HIP): built with plain g++, once more with AddressSanitizer and UBSan, and run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cwsl_digi_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]], ids=["plain", "asan-ubsan"])
def test_epoch_rule_matches_the_longhand_conditions(tmp_path, flags):
    exe = str(tmp_path / "record_kinds_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", CSRC, os.path.join(ROOT, "tests", "record_kinds_check.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout
    assert int(r.stdout.split()[1]) > 2_000_000                     # every state was visited
