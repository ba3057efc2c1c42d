"""bench.py --dump-outputs on hardware: what the timed path returned in its last step, written after the timed region."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_dump_outputs_is_the_last_timed_step_and_repeats(tmp_path):
    """`bench.py --tiny --steps 3 --dump-outputs DIR`: three timed steps, DIR/images.npy is the last one's edited latents (its hash is
    the line's latent_sha16), and a second run with the same arguments writes the same array (seeded inputs, deterministic engine)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    got = []
    for run in ("a", "b"):
        out = tmp_path / run
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--tiny", "--steps", "3", "--warmup", "1",
                            "--hash-latents", "--no-roofline-events", "--dump-outputs", str(out)],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.splitlines()[-1])
        assert line["steps"] == 3 and line["warmup"] == 1
        assert os.listdir(out) == ["images.npy"]
        x = np.load(out / "images.npy")
        assert x.dtype == np.float32 and x.shape == (1, 64, 64) and np.isfinite(x).all()
        assert hashlib.sha256(x.tobytes()).hexdigest()[:16] == line["config"]["latent_sha16"][0]
        got.append(x)
    assert np.array_equal(got[0], got[1])
