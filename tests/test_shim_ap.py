"""CPU: the shim's FT8 a-priori wrappers compile against the C ABI, and mergeApDecodes (C++) equals api.merge_ap_decodes (Python) on hand-made
records -- BP / OSD words win per ch_id, the a-priori words no BP / OSD record of the channel carries are kept, the order is (ch_id, entry)."""
import os
import subprocess

import numpy as np

import decodes_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "shim_ap_check.cpp")


def _rec(ch, entry, by_osd, word, st=0):
    r = np.zeros((), DR.DECODE_DTYPE)
    r["ch_id"], r["entry"], r["by_osd"], r["set"], r["ndup"] = ch, entry, by_osd, st, 1
    r["bits"] = np.frombuffer(bytes([word]) * 11 + b"\x20", np.uint8)
    return r


def test_wrappers_compile():
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", SRC])


def test_merge_helpers_agree(tmp_path):
    from cwsl_digi_amd.api import merge_ap_decodes
    exe = str(tmp_path / "shim_ap_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-DSHIM_AP_CHECK_MAIN", SRC, "-o", exe])
    dec = np.array([_rec(0, 0, 0, 1), _rec(0, 7, 1, 2), _rec(2, 3, 0, 3), _rec(5, 1, 0, 9)], DR.DECODE_DTYPE)
    ap = np.array([_rec(0, 4, 2, 2, 1),       # channel 0 has word 2 by OSD: dropped
                   _rec(0, 5, 2, 4),          # kept, between the channel's entries 0 and 7
                   _rec(1, 0, 2, 1),          # word 1 is channel 0's, not channel 1's: kept
                   _rec(2, 1, 2, 5, 1),       # kept, in front of channel 2's entry 3
                   _rec(2, 9, 2, 3)], DR.DECODE_DTYPE)       # channel 2 has word 3 by BP: dropped
    want = merge_ap_decodes(dec, ap)
    assert [(int(r["ch_id"]), int(r["entry"]), int(r["by_osd"])) for r in want] == [(0, 0, 0), (0, 5, 2), (0, 7, 1), (1, 0, 2), (2, 1, 2), (2, 3, 0), (5, 1, 0)]
    for d, a in ((dec, ap), (dec, ap[:0]), (dec[:0], ap), (dec[:0], ap[:0])):
        blob = np.array([len(d), len(a)], np.uint32).tobytes() + d.tobytes() + a.tobytes()
        got = subprocess.run([exe], input=blob, stdout=subprocess.PIPE, check=True).stdout
        assert got == merge_ap_decodes(d, a).tobytes()
