"""`python bench.py --gpus N` must measure N ranks by itself (the driver's command line has no torchrun).  Here the very
same launcher code (tvretrieval_amd/launch.py + bench.py main, entered through tests/bench_cpu_entry.py) starts 2 gloo
ranks on CPU, with the kernels replaced by tests/cpu_backend.py, and must print exactly one JSON line that says n_gpus = 2."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _run(argv, timeout=900, script="bench.py", **extra_env):
    env = dict(os.environ, PYTHONPATH=HERE + os.pathsep + ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **extra_env)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    path = os.path.join(ROOT, script) if script == "bench.py" else os.path.join(HERE, script)
    return subprocess.run([sys.executable, path] + argv, env=env, capture_output=True, text=True, timeout=timeout)


def test_bench_self_spawns_two_gloo_ranks():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--workload", "tiny", "--no-cpu-baseline", "--full"],
             script="bench_cpu_entry.py")
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert lines[-1].startswith("{") and sum(ln.startswith("{") for ln in lines) == 1, lines   # ONE result line, last
    res = json.loads(lines[-1])
    assert res["n_gpus"] == 2 and res["config"]["ranks_in_process_group"] == 2
    assert res["config"]["launcher"] == "bench.py self-spawn"
    assert len(res["config"]["videos_per_gpu"]) == 2 and sum(res["config"]["videos_per_gpu"]) == 300
    assert res["value"] > 0 and res["scaling"] == "strong"
    stages = res["breakdown_ms"]
    assert "exchange+merge_topk" in stages and "q2c_k6" in stages, stages
    # both rerank schemes get a number: the headline's (query owner) and the north_star-literal fully sharded one
    alt = res["extras"]["other_rerank_scheme"]
    assert alt["value"] > 0 and alt["collectives_per_pass"] == 4 and res["config"]["rerank"].startswith("query owner")
    assert res["config"]["collectives_fallback"] == 0


def test_bench_self_spawns_eight_gloo_ranks():
    """The driver's 8-GPU command line, rehearsed on CPU: `bench.py --gpus 8` through its own launcher, 8 gloo ranks, the
    300-video test corpus cut into 8 shards, both rerank schemes timed, one JSON line."""
    r = _run(["--gpus", "8", "--steps", "1", "--warmup", "0", "--workload", "tiny", "--no-cpu-baseline", "--full"],
             script="bench_cpu_entry.py", timeout=1500)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert lines[-1].startswith("{") and sum(ln.startswith("{") for ln in lines) == 1, lines
    res = json.loads(lines[-1])
    assert res["n_gpus"] == 8 and res["config"]["ranks_in_process_group"] == 8
    assert len(res["config"]["videos_per_gpu"]) == 8 and sum(res["config"]["videos_per_gpu"]) == 300
    assert min(res["config"]["videos_per_gpu"]) >= 37
    assert res["value"] > 0 and res["extras"]["other_rerank_scheme"]["value"] > 0


def test_bench_rank_failure_propagates():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--workload", "tiny"], timeout=300,
             script="bench_cpu_entry.py", XML_TEST_FAIL_RANK="1")
    assert r.returncode != 0


@pytest.mark.gpu
def test_bench_tiny_forced_sharded_on_gpu():
    """Same entry on the GPU box: the N > 1 code path through a real 1-rank RCCL group."""
    r = _run(["--gpus", "1", "--force-sharded", "--workload", "tiny", "--steps", "2", "--warmup", "1",
              "--no-cpu-baseline", "--full"])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["n_gpus"] == 1 and res["config"]["backend"] == "hip" and res["config"]["ranks_in_process_group"] == 1
    assert "exchange+merge_topk" in res["breakdown_ms"] or "topk_k8" in res["breakdown_ms"]
    assert res["config"]["collectives"].startswith("libxmlhip RCCL")


@pytest.mark.gpu
def test_bench_refuses_to_measure_fallback_collectives():
    """A C-ABI collective that fails its self-check must END an N > 1 run with a non-zero exit code -- a line that silently
    measured torch.distributed would be read as a measurement of csrc/collectives.hip -- unless --torch-collectives asked
    for that exchange on purpose (the line then carries collectives_fallback = 1)."""
    argv = ["--gpus", "1", "--force-sharded", "--workload", "tiny", "--steps", "1", "--warmup", "0", "--no-cpu-baseline"]
    r = _run(argv, XML_TEST_BREAK_CABI_COLLECTIVES="1")
    assert r.returncode != 0, r.stdout[-2000:]
    assert "Refusing to measure" in r.stderr and not any(ln.startswith("{") for ln in r.stdout.splitlines())
    r = _run(argv + ["--torch-collectives"], XML_TEST_BREAK_CABI_COLLECTIVES="1")
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert res["config"]["collectives_fallback"] == 1 and res["config"]["collectives"].startswith("torch.distributed")


def _dump_run(tmp_path, name, steps, warmup, script):
    import numpy as np
    out = tmp_path / name
    r = _run(["--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--workload", "tiny", "--dump-outputs", str(out)],
             script=script)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert lines[-1].startswith("{") and sum(ln.startswith("{") for ln in lines) == 1, lines
    res = json.loads(lines[-1])
    arrays = {p.stem: np.load(p) for p in sorted(out.glob("*.npy"))}
    return res, arrays


def _check_plain_run_and_dump(tmp_path, script):
    """A plain run times exactly --steps steps and measures nothing beside the headline (no stage breakdown, CPU baseline or
    extra legs); --dump-outputs writes the last timed step's lists, and the same arguments give the same arrays."""
    import numpy as np
    res1, a1 = _dump_run(tmp_path, "a", 1, 0, script)
    res2, a2 = _dump_run(tmp_path, "b", 2, 1, script)
    for res, steps in ((res1, 1), (res2, 2)):
        assert res["steps"] == steps and res["roofline"]["launches_timed"] == steps
        assert res["ms_per_step"] > 0 and abs(res["value"] - 64 * 1e3 / res["ms_per_step"]) < 1e-6 * res["value"]
        assert res["breakdown_ms"] == {} and res["cpu_baseline"] is None and "extras" not in res
    assert set(a1) == {"top_scores", "top_indices", "flat_scores", "flat_indices", "q2c_sample"}, sorted(a1)
    assert a1["top_scores"].shape == a1["top_indices"].shape == (64, 100)
    assert a1["flat_scores"].shape == a1["flat_indices"].shape == (64, 200)
    assert a1["q2c_sample"].shape == (64, 300)
    assert sum(a.nbytes for a in a1.values()) <= 64 << 20
    for name, a in a1.items():
        assert a.dtype == (np.float64 if name.endswith("indices") else np.float32), (name, a.dtype)
        assert np.array_equal(a, a2[name]), name
    assert (a1["top_indices"] >= 0).all() and (a1["top_indices"] < 300).all()
    assert (np.diff(a1["top_scores"], axis=1) <= 0).all()


def test_plain_run_and_dump_outputs(tmp_path):
    _check_plain_run_and_dump(tmp_path, "bench_cpu_entry.py")


def test_dump_outputs_refuses_several_ranks():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--workload", "tiny", "--dump-outputs", "unused"],
             script="bench_cpu_entry.py", timeout=120)
    assert r.returncode != 0 and "--dump-outputs needs a single-process run" in r.stderr


@pytest.mark.gpu
def test_plain_run_and_dump_outputs_on_gpu(tmp_path):
    _check_plain_run_and_dump(tmp_path, "bench.py")
