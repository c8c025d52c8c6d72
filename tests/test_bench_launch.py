"""CPU: bench.py's multi-rank launch contract.  `python bench.py --gpus N` with no launcher in the environment must produce N ranks
by itself (a child process under torch.distributed.run on 127.0.0.1) and print one JSON line whose n_gpus is N; a launcher that started
another number of ranks is refused.  `--dry` = gloo ranks and a stand-in gradient bucket through the engine's reduce path."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _clean_env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "2"
    return env


def test_bench_gpus_2_self_launches_two_ranks():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry", "--steps", "4", "--warmup", "1"],
                       env=_clean_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout                     # rank 0 only
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2 and r["ranks"] == 2 and r["steps"] == 4 and r["warmup"] == 1 and r["bucket_sums_correct"] is True
    assert r["config"]["parallelism"] == "dp2" and r["dry"] is True


def test_bench_dump_outputs_writes_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: rank 0 writes what the last timed step computed as float32 .npy files.  Dry step k fills rank r's bucket with
    r + 1 + k, so after --steps 4 on two ranks the reduced bucket holds (0 + 1 + 3) + (1 + 1 + 3) = 9 everywhere — and --steps set the count."""
    import numpy as np
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry", "--steps", "4", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], env=_clean_env(), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    r = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][0])
    assert r["steps"] == 4 and r["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path / "out")) == ["bucket.npy"]
    b = np.load(tmp_path / "out" / "bucket.npy")
    assert b.dtype == np.float32 and b.shape == (64 * 32 + 32,) and np.all(b == 9.0)


def test_bench_refuses_a_rank_count_other_than_requested():
    env = dict(_clean_env(), WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dry"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode != 0 and "refusing to report n_gpus" in (p.stderr + p.stdout)
    assert not [l for l in p.stdout.splitlines() if l.startswith("{")]


def _dry(*flags):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *flags, "--dry", "--steps", "3", "--warmup", "1"], env=_clean_env(),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_bench_ep_dry_two_ranks_padded_slabs():
    """`bench.py --gpus N --ep 2` = BASELINE configs[4] with the experts sharded over ep = 2 ranks (round-3 review, item 4).  Its gloo twin:
    DeepSpeed's group shapes, the host-side capacity agreement and a dispatch / combine round trip per step through ExpertParallel on every
    rank, so `--gpus 8 --ep 2` cannot fail on the driver's node for a reason this test could have caught."""
    r = _dry("--gpus", "2", "--ep", "2")
    assert r["n_gpus"] == 2 and r["config"]["parallelism"] == "ep2 x dp1" and r["bucket_sums_correct"] is True
    ep = r["ep"]
    assert ep["ep_size"] == 2 and ep["replicas"] == 1 and ep["round_trips_correct_on_every_rank"] is True and ep["variable_split"] is False
    assert ep["exchanges_per_step"] == 2.0 and ep["a2a_bytes_sent_per_exchange"] > 0


def test_bench_ep_dry_four_ranks_variable_split():
    """ep 2 x 2 replicas (the 8-GPU run's shape at half size) with routed rows only: two expert-parallel groups exchange side by side while
    the gradient bucket spans all four ranks."""
    r = _dry("--gpus", "4", "--ep", "2", "--ep-variable")
    assert r["n_gpus"] == 4 and r["ranks"] == 4 and r["config"]["parallelism"] == "ep2 x dp2" and r["bucket_sums_correct"] is True
    ep = r["ep"]
    assert ep["replicas"] == 2 and ep["variable_split"] is True and ep["round_trips_correct_on_every_rank"] is True


def test_bench_ep_must_divide_the_rank_count():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "3", "--ep", "2", "--dry"], env=_clean_env(), capture_output=True,
                       text=True, timeout=120)
    assert p.returncode != 0 and "does not divide" in (p.stderr + p.stdout)


def test_bench_eight_ranks_dry_the_drivers_own_commands():
    """The 8-GPU node's first contact cannot fail for a reason a CPU could have caught (round-4 review, item 6): the driver's exact command
    lines at the full rank count — `--gpus 8` and `--gpus 8 --ep 2 --ep-variable` (reference: scripts/train_medplib_icl.sh:15-43, 4 ranks there;
    train_ds_medplib.py:412-419) — through the self-launch, eight gloo ranks, the gradient bucket over all of them, four expert-parallel
    groups of two exchanging side by side; ONE line on stdout, n_gpus = ranks = 8."""
    r = _dry("--gpus", "8")
    assert r["n_gpus"] == 8 and r["ranks"] == 8 and r["config"]["parallelism"] == "dp8" and r["bucket_sums_correct"] is True
    r = _dry("--gpus", "8", "--ep", "2", "--ep-variable")
    assert r["n_gpus"] == 8 and r["ranks"] == 8 and r["config"]["parallelism"] == "ep2 x dp4" and r["bucket_sums_correct"] is True
    ep = r["ep"]
    assert ep["ep_size"] == 2 and ep["replicas"] == 4 and ep["variable_split"] is True and ep["round_trips_correct_on_every_rank"] is True
