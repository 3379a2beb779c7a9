"""bench.py's plain run on the GPU: the headline line alone (nothing of
--full in it), --steps honoured, and --dump-outputs writing the variables the
last timed step left as float32 .npy files within the size limit.  A small
FCN shape (2 x 64 x 96, the shape of tests/test_gpu_fcn.py) keeps it short;
conv6 / conv7 are still large enough to take the sampled path."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


@pytest.mark.gpu
def test_plain_run_headline_and_dump(dev, tmp_path):
    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--height", "64",
                        "--width", "96", "--batch", "2", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["unit"] == "images/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step describe the same three steps of 2 images
    assert line["value"] == pytest.approx(2 * 1e3 / line["ms_per_step"], rel=1e-3)
    for key in ("roofline", "loss_after", "miou_parity", "dp_mode", "data_pipeline", "inference", "c3_fcdensenet",
                "c5_deeplab", "cpu_baseline"):
        assert key not in line, key

    from oracle import models as M
    shapes = M.fcn_param_shapes(3, 2)
    files = sorted(os.listdir(out))
    assert set(files) == {k.replace("/", ".") + ".npy" for k in shapes} | {"loss.npy"}
    total = 0
    for k, s in shapes.items():
        a = np.load(out / (k.replace("/", ".") + ".npy"))
        total += a.nbytes
        assert a.dtype == np.float32 and a.ndim == 1 and np.isfinite(a).all(), k
        n = int(np.prod(s))
        assert a.size == n or (a.size < n and a.size >= 1 << 16), (k, a.size, n)
    loss = np.load(out / "loss.npy")
    total += loss.nbytes
    assert loss.dtype == np.float64 and np.isfinite(loss) and 0.0 < float(loss) < 50.0
    assert total <= 64 * 10 ** 6
    # a large variable is sampled, a small one whole
    assert np.load(out / "conv6.weights.npy").size < int(np.prod(shapes["conv6/weights"]))
    assert np.load(out / "conv1_1.weights.npy").size == int(np.prod(shapes["conv1_1/weights"]))
