"""GPU: the bench.py contract the round driver depends on -- exactly ONE line on stdout, a JSON record with the agreed fields,
exactly --steps timed steps, `roofline` and `cpu_baseline` objects under --full, and --dump-outputs (a small workload keeps this to a
few seconds)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_fields():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "tiny", "--steps", "20", "--warmup", "5", "--full",
                        "--min-seconds", "10"],
                       capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[:500]
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 5 and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and d["vs_baseline"] is None and "workload" in d["config"]
    assert d["timed_steps"] % 40 == 0 and d["timed_steps"] >= 200          # whole major-iteration periods, past the initial phase
    assert d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-3)
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"], abs=1e-3) and 0.0 < rf["frac"] < 1.0
    if "PYTEST_XDIST_WORKER" not in os.environ:  # (two timings of the same run: not under the contention soak, where the load changes between them)
        assert rf["avg_launch_ms"] < d["ms_per_step"]
    cpu = d["cpu_baseline"]
    assert cpu["kind"] == "port" and cpu["cores"] >= 1 and cpu["value"] > 0 and "sample" in cpu and cpu["unit"] == d["unit"]
    if "PYTEST_XDIST_WORKER" not in os.environ:  # (a rate comparison: not under the contention soak, where four processes share the GPU)
        assert d["value"] > cpu["value"]


def test_bench_launches_its_own_ranks():
    """`python bench.py --gpus N` needs no wrapper: it starts torch.distributed.run itself and relays rank 0's record.  With one
    GPU the launcher path is forced by --self-launch (one RCCL rank); asking for more GPUs than the box has ends, AFTER the
    launcher ran, in "N GPUs requested, V visible" and a non-zero exit code."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--self-launch", "--workload", "tiny", "--steps", "20",
                        "--warmup", "5", "--no-cpu-baseline", "--no-convergence-run"], capture_output=True, text=True, cwd=ROOT, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[:500]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["rccl_nranks"] == 1 and d["value"] > 0
    from cuopt_amd import capi
    visible = capi.device_count()
    if visible < 16:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(visible + 1), "--workload", "tiny"],
                           capture_output=True, text=True, cwd=ROOT, timeout=900)
        assert r.returncode != 0 and not r.stdout.strip()
        assert "%d GPUs requested, %d visible" % (visible + 1, visible) in r.stderr


@pytest.mark.parametrize("workload, lps", [("tiny", 0), ("c2_batch4", 4), ("c5_batch64", 64)])
def test_plain_run_times_the_steps_and_dumps_what_they_computed(tmp_path, workload, lps):
    """without --full: the headline line alone (the legs of --full are null), exactly --steps timed steps where the workload counts
    steps, and --dump-outputs writes the solution of the last timed step -- the same bits in two runs with the same arguments"""
    dumps = []
    for run in range(2):
        out = tmp_path / ("run%d" % run)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", workload, "--steps", "70", "--warmup", "5",
                            "--dump-outputs", str(out)], capture_output=True, text=True, cwd=ROOT, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
        assert len(lines) == 1, r.stdout[:500]
        d = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in d, key
        assert d["metric"] == "pdlp_iterations_per_sec" and d["higher_is_better"] is True and d["dtype"] == "f64" and d["ms_per_step"] > 0
        assert d["cpu_baseline"] is None
        if workload.startswith("c5_batch"):  # (the small-LP batch times re-solves to 1e-4, not a step count; its roofline is a model of that rate)
            assert d["thread_pool"] is None
        else:
            assert d["timed_steps"] == 70 and d["roofline"] is None and d["time_to_1e-4"] is None
        files = sorted(os.listdir(out))
        prefixes = ["lp%02d_" % l for l in range(lps)] if workload.startswith("c2_batch") else ["lp%04d_" % l for l in range(lps)] if lps else [""]
        names = ("primal_solution", "dual_solution", "reduced_cost", "result_scalars")
        assert files == sorted(pre + n + ".npy" for pre in prefixes for n in names), files[:8]
        arrays = {f: np.load(out / f) for f in files}
        assert all(a.dtype == np.float64 and a.ndim == 1 for a in arrays.values())
        assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
        assert all(np.isfinite(a).all() for a in arrays.values())
        if not workload.startswith("c5_batch"):  # result_scalars[0] = steps_taken: the warm-up done and the timed steps
            assert arrays[prefixes[0] + "result_scalars.npy"][0] == d["warmup_done"] + 70
        dumps.append(arrays)
    for f in dumps[0]:
        np.testing.assert_array_equal(dumps[0][f], dumps[1][f], err_msg=f)
