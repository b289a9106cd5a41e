"""-m gpu: bench.py end to end on a small frame.  A plain run prints the headline line and nothing it does not need; --full adds
the legs beside it (the oracle check, the light pipe, the measured copy ceiling, the host-to-host legs).  Both runs export the
same words, and --full finds them equal to the oracle's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--size", "1024x768"]


def _bench(extra, dump_dir, timeout):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + ["--dump-outputs", str(dump_dir)] + extra,
                         cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["unit"] == "MPix/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 2 and line["warmup"] == 1
    assert line["value"] == pytest.approx(1024 * 768 / 1e6 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    return line, np.load(os.path.join(str(dump_dir), "export_rgba.npy"))


def test_plain_run_is_the_headline_and_full_adds_the_legs(tmp_path):
    plain, plain_words = _bench([], tmp_path / "plain", timeout=300)
    assert "verified" not in plain and "cpu_baseline" not in plain
    cfg = plain["config"]
    assert cfg["light_pipe"] is None and cfg["default_diffuse"] is None and cfg["host_to_host_ms"] is None
    assert plain["roofline"]["peak_measured"] is None
    assert cfg["kernels_ms_per_step"] and plain["roofline"]["kernel"] in cfg["kernels_ms_per_step"]

    full, full_words = _bench(["--full", "--no-cpu-baseline"], tmp_path / "full", timeout=600)
    assert full["verified"] is True and full["verify"]["mismatches"] == 0
    cfg = full["config"]
    assert cfg["light_pipe"]["ms_per_step"] > 0 and cfg["default_diffuse"]["ms_per_step"] > 0
    assert cfg["host_to_host_ms"] > 0
    assert full["roofline"]["peak_measured"]["copy_GBs"] > 0

    assert plain_words.shape == (768, 1024, 4)
    np.testing.assert_array_equal(plain_words, full_words)
