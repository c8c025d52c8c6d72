"""GPU: a plain `bench.py` run prints the headline and what the timed steps recorded, nothing that needs work of its own after them;
`--full` turns that work back on (here the unshared roofline steps and the upsampler roofline, the cheap part of it), at 2 decoder layers."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline_upsampler", "lora_stage3", "configs", "decode", "cpu_baseline", "parity")


def _run(extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--layers", "2", "--steps", "3", "--warmup", "1"] + extra,
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_plain_line_is_the_headline(dev):
    r = _run([])
    assert r["metric"] == "train samples/sec (img+64tok)" and r["unit"] == "samples/s" and r["higher_is_better"] is True and r["dtype"] == "bf16"
    assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0
    assert abs(r["value"] - 8 / (r["ms_per_step"] * 1e-3)) < 0.02 * r["value"]
    assert not [k for k in FULL_ONLY if k in r]
    assert r["roofline"]["kernel"] and "sample" not in r["roofline"] and r["roofline_timed_region"] is None     # the timed steps' own figure


def test_bench_full_adds_the_unshared_roofline_and_the_upsampler(dev):
    r = _run(["--full", "--no-cpu-baseline", "--no-lora-line", "--no-secondary"])
    assert r["steps"] == 3 and r["ms_per_step"] > 0
    assert "sample" in r["roofline"] and r["roofline_timed_region"]["kernel"]
    assert r["roofline_upsampler"]["sam1024"]["us_per_launch"] > 0
