"""GPU: `bench.py --dump-outputs DIR` on the default line (BASELINE configs[3]) at 2 decoder layers.  The files are what the LAST timed step
computed — every loss of the dict the model returned and the trainable parameters after its AdamW update — in float32 and within 64 MB, and two
runs with the same arguments (seeded inputs and weights) write the same numbers, which is what lets two builds be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--layers", "2", "--steps", "3", "--warmup", "1",
                        "--roofline-steps", "0", "--no-cpu-baseline", "--no-lora-line", "--no-secondary", "--no-kernel-timer", "--no-live-traffic",
                        "--dump-outputs", str(out_dir)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}


def test_bench_dump_outputs_of_the_default_line(dev, tmp_path):
    from medplib_amd.model.medplib import LOSS_KEYS
    r, a = _run(tmp_path / "a")
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    assert sorted(a) == sorted(LOSS_KEYS + ["trainable_params"])
    assert all(v.dtype == np.float32 and np.all(np.isfinite(v)) for v in a.values())
    assert sum(os.path.getsize(tmp_path / "a" / f"{k}.npy") for k in a) <= 64 * 10**6
    assert float(a["loss"]) == r["loss_last"]                       # the last timed step's loss, as the result line reports it
    n = r["config"]["trainable_params"]
    assert a["trainable_params"].shape == (min(n, 8 * 10**6),)
    _, b = _run(tmp_path / "b")
    for k in LOSS_KEYS:
        np.testing.assert_allclose(b[k], a[k], rtol=1e-5, atol=0, err_msg=k)
    np.testing.assert_allclose(b["trainable_params"], a["trainable_params"], rtol=0, atol=1e-6)
