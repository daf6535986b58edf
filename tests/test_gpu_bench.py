"""bench.py's plain run on the GPU: the headline line only (roofline, CPU baseline and the other configurations need --full),
and --dump-outputs writes the mels of the last timed run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_measures_the_headline_and_dumps_the_mels(tmp_path):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["metric"] == "mel_frames_per_sec_50step_dpmsolver" and d["unit"] == "mel-frames/s" and d["higher_is_better"] is True
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["dtype"].startswith("bf16x3")
    assert d["value"] == pytest.approx(8 * 1024 / (d["ms_per_step"] * 1e-3), rel=1e-6)
    assert not {"roofline", "cpu_baseline", "extra"} & set(d)
    mel = np.load(tmp_path / "mel.npy")
    assert mel.dtype == np.float32 and mel.shape == (8, 80, 1024) and np.isfinite(mel).all()
