"""GPU: decode_harvest_kernel (csrc/harvest_kernels.hpp) on synthetic records -- crowded channels, one word on 600 entries, poisoned FT4
slots, 600 channels with decodes everywhere -- so that every carry between two passes of 256 (slots, listed words, survivors, channels) is
taken.  tests/harvest_kernel_check.hip drives the kernel through harvest_launch, the launch sequence of cwslg_fetch_decodes, once for all
cases of tests/harvest_kernel_cases.py in one child process; every comparison is byte for byte against tests/decodes_ref.py: n_total, the
records, counts[], offsets[] and the 0xAB guard behind each block."""
import subprocess

import numpy as np
import pytest

import decodes_ref as DR
import harvest_kernel_cases as K

pytestmark = pytest.mark.gpu
RUN_TIMEOUT_S = 60.0                                                    # the 45 cases took 0.34 s on an MI355X, device start-up included: a safeguard for a loaded machine, not a measurement


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    """family -> [(counts, offsets, out)] as the kernel left them: the program built, all cases written, ONE run.  A non-zero exit or the time
    limit fails the fixture (and with it every test of this module) and nothing else is started."""
    tmp = tmp_path_factory.mktemp("harvest_kernel")
    exe = K.build_check_program(tmp)
    cases = K.all_cases()
    fin, fout = tmp / "cases.bin", tmp / "results.bin"
    K.write_cases(fin, [c for _, _, c in cases])
    try:
        p = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=RUN_TIMEOUT_S)
    except subprocess.TimeoutExpired:
        pytest.fail(f"harvest_kernel_check did not finish within {RUN_TIMEOUT_S} s")
    if p.returncode != 0:
        pytest.fail(f"harvest_kernel_check exit {p.returncode}: {p.stdout[-500:]} {p.stderr[-2000:]}")
    got = K.read_results(fout, [c for _, _, c in cases])
    out = {}
    for (name, i, _), g in zip(cases, got):
        assert len(out.setdefault(name, [])) == i
        out[name].append(g)
    return out


@pytest.mark.parametrize("name", list(K.FAMILIES))
def test_kernel_against_decodes_ref(results, name):
    """Every case of the family: the three blocks equal what decodes_ref says, to the byte; the first differing record is shown with its case."""
    diffs = [K.first_difference(case, got, want) for case, got, want in zip(K.family(name), results[name], K.expected(name))]
    assert len(results[name]) == len(K.family(name)) > 0
    assert not any(diffs), [d for d in diffs if d]


def test_hand_written_answers(results):
    """The hand-written cases against the records written out literally in harvest_kernel_cases: decodes_ref is not the only judge."""
    n = 0
    for name in K.FAMILIES:
        for case, (counts, offsets, out) in zip(K.family(name), results[name]):
            if case["literal"] is None:
                continue
            want = np.array(case["literal"], DR.DECODE_DTYPE) if case["literal"] else np.zeros(0, DR.DECODE_DTYPE)
            got = out[K.HEAD_WORDS:K.HEAD_WORDS + K.REC_WORDS * len(want)].view(DR.DECODE_DTYPE)
            assert int(out[0]) == len(want) == int(counts[0]) and got.tobytes() == want.tobytes(), (case["name"], int(out[0]), got, want)
            n += 1
    assert n >= 9
