"""bench.py's contract with the runs that compare builds: a plain run measures the headline and nothing else (--full adds the rest), and
--dump-outputs writes the last timed step's outputs, identical from run to run for the same arguments."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*argv, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=timeout, env=env, cwd=ROOT)


def test_verify_needs_full():
    p = _bench("--verify", "2", "--dry-run")
    assert p.returncode == 2 and "only a --full run" in p.stderr, p.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    dumps = []
    for k in range(2):
        d = tmp_path / f"dump{k}"
        p = _bench("--gpus", "1", "--slots", "32", "--steps", "2", "--warmup", "1", "--dump-outputs", str(d))
        assert p.returncode == 0, p.stderr[-3000:]
        line = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["mode"].startswith("exact")
        assert "fast" not in line and line["cpu_baseline"] is None and line["verify"] == {}      # --full's records only
        files = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(str(d / "*.npy"))}
        assert sorted(files) == ["audio_f32", "candidates", "frame_i16", "frame_meta"]
        assert all(v.dtype in (np.float32, np.float64) for v in files.values())
        assert sum(v.nbytes for v in files.values()) <= 64 << 20
        assert files["audio_f32"].shape[0] == files["frame_i16"].shape[0] == 16 and np.abs(files["audio_f32"]).max() > 0
        dumps.append(files)
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name].view(np.uint8), dumps[1][name].view(np.uint8)), name
