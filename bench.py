#!/usr/bin/env python
"""PDLP iterations/sec on the BASELINE.json workloads, MI355X.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--workload c3|c2|tiny|hard]
  N > 1: one process per GPU over RCCL.  Either the caller launches them (`python -m torch.distributed.run --nproc-per-node N
  ... bench.py --gpus N ...`: WORLD_SIZE / RANK / LOCAL_RANK in the environment) or plain `python bench.py --gpus N` starts
  that launcher itself (127.0.0.1, a free port) and relays the one JSON line of rank 0; `--self-launch` forces the launcher
  for N = 1 too (one RCCL rank: `rccl_nranks` 1).  More GPUs requested than visible: every rank stops with
  "N GPUs requested, V visible" and the exit code is non-zero -- there is no fallback to fewer devices.

A "step" is ONE PDLP iteration (one accepted PDHG step), including its amortised share of
the major-iteration work (averages, 2 convergence evaluations, restart logic every 40 steps): the
timed region is `cuoptamd_solver_advance(K)` on a solver whose problem is already resident in HBM, with
all six tolerances at 0 so that no early exit can shorten the run (the reference's own device:
cpp/tests/linear_programming/pdlp_test.cu:145-148).  N > 1 shards the SAME LP (strong scaling): every rank holds a row block
and a column block of A, the slices of xbar and y' are all-gathered over RCCL each step (owner-computes dataflow, the default;
CUOPT_AMD_SHARD_DATAFLOW / CUOPT_AMD_SHARD_TRANSPORT select the others, `config.parallelism` names what ran).

Prints ONE JSON line (rank 0).  The timed region is exactly --steps iterations (`timed_steps`; --min-seconds S > 0 lengthens it
to at least S seconds) and `ms_per_step` is its wall time per iteration; `value` = 1000 / ms_per_step.

A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the line; `roofline`, `cpu_baseline` and
`time_to_1e-4` are null there.  --full adds the rest, each leg a run of its own after the timed region: `roofline` is for the
dominant kernel (the fused CSR SpMV + dual projection), timed with HIP events on the solver's stream by pdlpdev_time_kernel;
`cpu_baseline` is the C oracle's PDLP loop (oracle/pdlp_oracle.c, kind "port") on the same LP with a bounded iteration budget;
`time_to_1e-4` a solve at the default tolerances, set-up included; the shader clock sampled during the timed region; and for the
batch workloads the single-LP rate, the thread-pool leg and the reference's dual simplex.

--dump-outputs DIR: what the timed path handed its caller after its last step, as DIR/<name>.npy (float64): primal_solution,
dual_solution, reduced_cost (cuoptamd_solver_get_solution, rank 0) and result_scalars (RESULT_FIELDS, in that order); the batch
workloads write lp<index>_<name> per LP.  The inputs are seeded, so two runs with the same arguments compare output for output.
Above 64 MB in all, every large array is cut to the same fixed, seeded sample of its entries.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E peak, /opt/skills/guides/MI355X_MICROARCH.md

# --dump-outputs: the result fields written as result_scalars.npy (the timings are left out: they differ from run to run)
RESULT_FIELDS = ("steps_taken", "attempted_steps", "num_restarts", "primal_objective", "dual_objective", "gap", "relative_gap",
                 "l2_primal_residual", "l2_dual_residual", "l2_relative_primal_residual", "l2_relative_dual_residual", "step_size",
                 "primal_weight")
DUMP_BUDGET_BYTES = 60 << 20  # (under the 64 MB the files may take, .npy headers included)

# The clock warm-up's batches run a number of iterations that depends on the clocks; the solvers then start again from their fresh
# state and run --warmup (rounded up to whole periods) plus these major-iteration periods untimed, the same count in every run.  That
# is as far in as the timed steps started behind the clock warm-up before (4 batches of 5 periods): on C3 the adaptive step size
# rejects ~1 % of the attempts of iterations 200-2200 and next to none after iteration 1000, and the headline never included them.
SETTLE_PERIODS = 20


def solver_outputs(result, x, y, rc, prefix=""):
    """the arrays a caller of the timed path receives: the solution vectors and the result's numbers"""
    return {prefix + "primal_solution": x, prefix + "dual_solution": y, prefix + "reduced_cost": rc,
            prefix + "result_scalars": np.array([float(result[k]) for k in RESULT_FIELDS])}


def dump_outputs(out_dir, arrays):
    """writes every array as out_dir/<name>.npy, float64.  When they hold more than DUMP_BUDGET_BYTES, the arrays above 1 MB are all
    cut to the same share of their entries, at positions drawn with a fixed seed from the array's length alone: the same
    positions in every run with the same arguments."""
    os.makedirs(out_dir, exist_ok=True)
    arrays = {k: np.ascontiguousarray(v, dtype=np.float64).ravel() for k, v in arrays.items()}
    large = {k for k, a in arrays.items() if a.nbytes > (1 << 20)}
    small_bytes = sum(a.nbytes for k, a in arrays.items() if k not in large)
    large_bytes = sum(arrays[k].nbytes for k in large)
    share = 1.0 if small_bytes + large_bytes <= DUMP_BUDGET_BYTES else (DUMP_BUDGET_BYTES - small_bytes) / large_bytes
    for name, a in arrays.items():
        if name in large and share < 1.0:
            keep = max(1, int(len(a) * share))
            a = a[np.sort(np.random.default_rng(len(a)).choice(len(a), size=keep, replace=False))]
        np.save(os.path.join(out_dir, name + ".npy"), a)


def reference_dual_simplex_block(root, cutoff_s=15.0):
    """The reference's own CPU dual simplex (oracle/_ref: cpp/src/dual_simplex compiled in place, 1 thread) as the
    objective oracle on the configurations it can finish: C1 (afiro), one C5 input (50v-10 LP relaxation) and C2 with a
    wall-clock cutoff; C3 is not attempted."""
    import json as _json
    out = {}
    try:
        from oracle import refbind
        if not refbind.available():
            return {"note": "oracle/_ref is not built on this box"}
        from cuopt_amd import synthetic
        gold = _json.load(open(os.path.join(root, "tests", "golden", "problems.json")))
        cases = [("C1 afiro", gold["afiro"], 0.0), ("C5 50v-10 LP relaxation", gold["mip-50v-10-free-bound-relaxation"], 0.0),
                 ("C2 S(1e5,1e5,10,seed=1)", synthetic.generate(**synthetic.CONFIGS["c2"]), cutoff_s)]
        for name, q, limit in cases:
            t0 = time.perf_counter()
            r = refbind.dual_simplex(q, time_limit=limit)
            out[name] = dict(status=r["status"], objective=r["objective"] if np.isfinite(r["objective"]) else None, pivots=r["iterations"],
                             wall_s=round(time.perf_counter() - t0, 3), threads=1,
                             cutoff_s=limit if limit else None)
        out["C3 S(1e6,1e6,10,seed=2)"] = "not attempted: the C2 run above is the bound (10x the rows, dense LU of the basis)"
    except Exception as e:  # the block is informative: never fail the bench line over it
        out["error"] = repr(e)
    return out


def shader_clock_mhz():
    """current sclk of GPU 0 as rocm-smi reports it (None when the tool is absent): printed at both ends of the timed region so that a
    box running below its steady clocks shows up in the line (round 4: 11 % between two boxes on c3x10, unexplained)"""
    import re
    import subprocess
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=20).stdout
        card = next(iter(json.loads(out).values()))
        for k, v in card.items():
            if "sclk" in k.lower():
                m = re.search(r"(\d+)\s*mhz", str(v).lower())
                if m:
                    return int(m.group(1))
    except Exception:
        pass
    return None


def cpu_baseline_block(p):
    """the C oracle's PDLP loop on the same LP, bounded iteration budget (kind "port": cuOpt ships no CPU PDLP).  Thread counts
    16 / 32 / 64 / 128 are tried once each on a 12-iteration calibration run and the best one gets the ~20 s sample; box cores and
    threads used are both reported."""
    # threads pinned to neighbouring cores; the oracle touches its arrays first from the threads that work on them
    # (oracle/pdlp_oracle.c dalloc / copy_rows_*), so a multi-socket box reads mostly local memory
    os.environ.setdefault("OMP_PROC_BIND", "close")
    os.environ.setdefault("OMP_PLACES", "cores")
    from oracle import orcbind
    if not orcbind.available():
        return None
    try:
        box_cores = len(os.sched_getaffinity(0))
    except AttributeError:
        box_cores = os.cpu_count() or 1
    # The GPU boxes run this command inside a cgroup with a CPU-time QUOTA (measured: cpu.max = "1600000 100000" = 16 CPUs' worth on a
    # 2 x 64-core EPYC 9575F with 256 hardware threads visible): more threads than the quota are throttled by the scheduler -- the
    # oracle's loop ran at 33 / 18 / 7.7 / 2.9 it/s with 16 / 32 / 64 / 128 threads while nr_throttled climbed (profiles/
    # r06_cpu_baseline_threads.txt).  That, not first touch or binding, is the "negative scaling" of the round-5 line: the baseline uses
    # what the box grants.
    quota_cores = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            quota_cores = max(1, int(float(q) / float(per)))
    except Exception:
        pass
    usable = min(box_cores, quota_cores) if quota_cores else box_cores
    sweep = {}
    for t in sorted({max(1, min(t, usable)) for t in (usable // 2, usable, 16, 32, 64, 128)}):
        o = orcbind.solve(p, tol=0.0, iteration_limit=12, num_threads=t)
        sweep[t] = o["steps_taken"] / max(o["loop_seconds"], 1e-9)
    cores = max(sweep, key=sweep.get)
    # (all 12 calibration steps are major iterations: an under-estimate of the rate, so the sample is bounded)
    budget = int(min(max(20.0 * sweep[cores], 40), 4000))
    o = orcbind.solve(p, tol=0.0, iteration_limit=budget, num_threads=cores)
    cpu = dict(value=round(o["steps_taken"] / o["loop_seconds"], 3), unit="iterations/s", cores=cores,
               box_cores=box_cores, cgroup_cpu_quota_cores=quota_cores, kind="port",
               thread_sweep_calibration_its_per_s={str(k): round(v, 2) for k, v in sweep.items()},
               sample="oracle/pdlp_oracle.c PDLP loop (OpenMP, %d threads; the box shows %d hardware threads and grants a CPU quota of %s), %d iterations of the same "
               "LP: loop %.2fs + setup %.2fs" % (cores, box_cores, "%d cores" % quota_cores if quota_cores else "all of them", o["steps_taken"], o["loop_seconds"],
                                               o["solve_seconds"] - o["loop_seconds"]))
    cpu["reference_dual_simplex"] = reference_dual_simplex_block(ROOT)
    return cpu


def batch_line(args, p, cfg, K, local_rank, record_fd, t_gen):
    """--workload c3_batch<K>: K LPs over ONE matrix and objective (different variable bounds: the MIP heuristics' re-solve pattern,
    BASELINE config 5 at the headline size) advance in lockstep (cuoptamd_batch_*; kernels_batch.hip).  value = AGGREGATE PDLP
    iterations/s over the K LPs; every LP's trajectory is bit-identical to its own single solve (tests/test_shared_batch_gpu.py)."""
    from cuopt_amd import capi, synthetic
    m, n, nnz = p["m"], p["n"], int(len(p["values"]))
    rng = np.random.default_rng(8)

    def bounds(l):
        lb, ub = np.array(p["lb"], float), np.array(p["ub"], float)
        if l:
            for j in rng.choice(n, size=n // 10, replace=False):
                ub[j] = p["x_star"][j] + 0.3 * rng.random()
        return lb, ub
    # (BENCH_USE_GRAPH=0: plain launches instead of replay graphs -- rocprofv3 7.2 falls over a process that instantiates a second
    #  family of graphs after destroying a first; the counter passes of scripts/gpu_session.sh pmc:c3_batch8 set it)
    graph = int(os.environ.get("BENCH_USE_GRAPH", "1"))
    parent = capi.Solver(p, mode=1, tol=0.0, device=local_rank, use_graph=graph)
    setup_s = parent.advance(0)["setup_seconds"]
    dev = parent.device
    if graph:
        dev.call("prepare_graphs")
    period = max(int(parent.hyper.major_iteration), 1)
    pre = ((max(args.warmup, 2 * period, int(parent.hyper.min_iteration_restart) + period) + period - 1) // period) * period
    single = None
    if args.full:
        # the single solve's rate in this very process (the yardstick of the aggregate)
        parent.advance(pre)
        rates = []
        for _ in range(4):
            dev.call("synchronize")
            t0 = time.perf_counter()
            parent.advance(25 * period)
            dev.call("synchronize")
            rates.append(25 * period / (time.perf_counter() - t0))
        single = max(rates[1:])
        parent.reset(tol=0.0, use_graph=graph)
    sets = [bounds(l) for l in range(1, K)]
    t0 = time.perf_counter()
    clones = [parent.clone(lb, ub) for lb, ub in sets]
    clone_s = (time.perf_counter() - t0) / max(K - 1, 1)
    batch = capi.SharedMatrixBatch([parent] + clones)
    layout = dev.layout()
    batch.advance(pre)
    fixed_pre = pre
    warm_rates, warm_wall = [], 0.0
    while True:
        dev.call("synchronize")
        tb = time.perf_counter()
        batch.advance(5 * period)
        dev.call("synchronize")
        dt = time.perf_counter() - tb
        pre += 5 * period
        warm_wall += dt
        warm_rates.append(5 * period / dt)
        if (len(warm_rates) >= 3 and all(abs(warm_rates[-i] - warm_rates[-i - 1]) <= 0.02 * warm_rates[-i] for i in (1, 2))) or warm_wall > 4.0:
            break
    # (the number of clock warm-up batches depends on the clocks: every LP starts again from its fresh state in a new batch and runs a
    # fixed warm-up (SETTLE_PERIODS), so that the timed steps -- and what --dump-outputs writes -- are the same iterations in every run)
    batch.close()
    for s in [parent] + clones:
        s.reset()
    batch = capi.SharedMatrixBatch([parent] + clones)
    if graph:
        dev.call("prepare_graphs")
    pre = fixed_pre + SETTLE_PERIODS * period
    batch.advance(pre)
    timed_steps = max(args.steps, 1)
    if args.min_seconds > 0:
        timed_steps = max(timed_steps, int(np.ceil(args.min_seconds * warm_rates[-1] / period)) * period)
    attempts_before = sum(r["attempted_steps"] for r in batch.advance(0))
    dev.call("synchronize")
    t0 = time.perf_counter()
    rs = batch.advance(timed_steps)
    dev.call("synchronize")
    elapsed = time.perf_counter() - t0
    assert all(r["status"] == 0 and r["steps_taken"] == pre + timed_steps for r in rs), [(r["status_name"], r["steps_taken"]) for r in rs]
    attempts = sum(r["attempted_steps"] for r in rs) - attempts_before
    if args.dump_outputs:
        arrays = {}
        for l, (r, (x, y, z)) in enumerate(zip(rs, batch.solutions())):
            arrays.update(solver_outputs(r, x, y, z, prefix="lp%02d_" % l))
        dump_outputs(args.dump_outputs, arrays)
    roofline = None
    if args.full:
        kernels = batch.time_kernels(20)
        bytes_alg = {
            # the matrix once, every gathered vector entry of every LP once, the per-LP epilogue streams, the interleaved copy of y'
            "a_dual": 12 * nnz + 4 * (m + 1) + K * (8 * n + 8 * (4 * m + 2 * m)) + 8 * K * m,
            "at_step": 12 * nnz + 4 * (n + 1) + K * (8 * m + 8 * (3 * n + n)),
            "primal": K * 8 * (6 * n + 3 * n),  # x,c,AtY,lb,ub,sum_x r ; x',sum_x w ; xbar interleaved w
        }
        dom = "a_dual" if kernels["a_dual"] >= kernels["at_step"] else "at_step"
        achieved = bytes_alg[dom] / (kernels[dom] * 1e-3) / 1e9
        ksum = sum(kernels.values())
        floor_k = 24 * nnz + 4 * (m + n + 2) + K * 8 * (14 * n + 7 * m) + 2 * 8 * K * (n + m)
        per_attempt_ms = 1e3 * elapsed / max(attempts / K, 1)
        roofline = dict(bound="hbm", kernel="kb_" + dom + "<%d>" % K, achieved=round(achieved, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                        frac=round(achieved / HBM_PEAK_GBS, 4), traffic=None, algorithmic_bytes_per_launch=bytes_alg[dom],
                        avg_launch_ms=round(kernels[dom], 5), per_kernel_ms={k: round(v, 5) for k, v in kernels.items()},
                        per_kernel_gbs={k: round(bytes_alg[k] / (kernels[k] * 1e-3) / 1e9, 1) for k in bytes_alg},
                        attempt_kernels_ms=round(ksum, 5), ms_per_lockstep_attempt=round(per_attempt_ms, 5),
                        attempt_kernels_over_ms_per_attempt=round(ksum / per_attempt_ms, 4),
                        lockstep_iteration_floor_bytes=floor_k,
                        iteration_frac_of_peak=round(floor_k * (timed_steps / elapsed) / 1e9 / HBM_PEAK_GBS, 4),
                        floor_note="fused floor of a lockstep iteration: the matrix twice (A, A^T) ONCE for all LPs, every LP's own 14 n + 7 m "
                                   "vector streams, the two interleaved gather vectors written and read once")
    batch.close()
    for c in clones:
        c.close()
    parent.close()
    # ---- wall clock to the default 1e-4 verdicts, set-ups included: one set-up + K - 1 clones + the lockstep solve against K
    # solves one after the other, each with its own set-up (what K calls of cuOptSolve cost)
    conv = None
    if args.full and not args.no_convergence_run:
        all_sets = [bounds(0)] + sets
        t0 = time.perf_counter()
        par = capi.Solver(dict(p, lb=all_sets[0][0], ub=all_sets[0][1]), mode=1, device=local_rank)
        cl = [par.clone(lb, ub) for lb, ub in all_sets[1:]]
        bt = capi.SharedMatrixBatch([par] + cl)
        rb = bt.advance()
        par.device.call("synchronize")
        wall_batch = time.perf_counter() - t0
        bt.close()
        for c in cl:
            c.close()
        par.close()
        t0 = time.perf_counter()
        rs1 = []
        for lb, ub in all_sets:
            s1 = capi.Solver(dict(p, lb=lb, ub=ub), mode=1, device=local_rank)
            rs1.append(s1.advance())
            s1.close()
        wall_seq = time.perf_counter() - t0
        conv = dict(statuses=[r["status_name"] for r in rb], iterations=[r["steps_taken"] for r in rb],
                    same_as_the_single_solves=all(a["steps_taken"] == b["steps_taken"] and a["primal_objective"] == b["primal_objective"] for a, b in zip(rb, rs1)),
                    wall_s_lockstep=round(wall_batch, 4), wall_s_one_after_the_other=round(wall_seq, 4), ratio=round(wall_seq / wall_batch, 3))
    cpu = cpu_baseline_block(p) if args.full and not args.no_cpu_baseline else None
    if cpu is not None:
        cpu["note"] = "the oracle solves one LP at a time: its aggregate over K LPs is this rate"
    info = capi.device_info(local_rank)
    out = {
        "metric": "pdlp_iterations_per_sec", "value": round(K * timed_steps / elapsed, 2), "unit": "iterations/s (aggregate over %d LPs)" % K,
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "timed_steps": timed_steps, "warmup_done": pre,
        "ms_per_step": round(1e3 * elapsed / timed_steps, 5), "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic",
        "config": {"workload": "%s: %d LPs over the matrix and objective of the base workload (synthetic random sparse LP S(m=%d,n=%d,k=%d,seed=%d), nnz=%d); LP 0 = the base LP, "
                               "the others with a tenth of the upper bounds tightened (seeded); lockstep batch, Stable2 preset, tolerances 0 (fixed "
                               "iteration budget)" % (args.workload, K, m, n, cfg["k"], cfg["seed"], nnz),
                   "rows": m, "cols": n, "nnz": nnz, "lps": K, "parallelism": "single GPU, %d LPs in lockstep" % K},
        "single_lp_its_per_s_same_process": None if single is None else round(single, 1),
        "aggregate_over_single": None if single is None else round(K * timed_steps / elapsed / single, 3),
        "clone_seconds_per_lp": round(clone_s, 4),
        "roofline": roofline, "cpu_baseline": cpu, "time_to_1e-4": conv, "spmv_layout": layout, "attempted_steps": attempts, "setup_seconds": round(setup_s, 4),
        "generate_seconds": round(t_gen, 2), "device": info["name"], "compute_units": info["compute_units"],
    }
    sys.stdout.flush()
    os.write(record_fd, (json.dumps(out) + "\n").encode())


def small_batch_line(args, K, local_rank, record_fd):
    """--workload c5_batch<K>: BASELINE config 5 at branch-and-bound scale.  K copies of the 50v-10 LP relaxation (datasets/mip/
    50v-10-free-bound.mps, 233 x 2013, 2745 nonzeros: tests/golden/problems.json) are K open nodes of a branch-and-bound tree: every
    round tightens, in each node, the bound of one integer variable that the node's relaxation left fractional (down-branch in even
    nodes, up-branch in odd ones) and re-solves from the previous primal / dual -- cpp/src/mip/relaxed_lp/relaxed_lp.cu:74-108.  The K
    persistent solvers advance as ONE small-LP batch (cuoptamd_batch_* over resident solvers: a workgroup per LP, one launch per phase
    of the loop).  value = aggregate PDLP iterations/s inside the batch's advance calls; lps_per_sec = re-solves per second for the
    whole pipeline (reset + advance + solution read-back).  Beside it: the same re-solves through a pool of 16 host threads, one
    solver and one stream each (what cuoptamd_batch_solve did before round 6), and the reference's dual simplex (1 thread)."""
    import concurrent.futures
    import ctypes as C
    from cuopt_amd import capi
    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "problems.json")))["mip-50v-10-free-bound-relaxation"]
    dec = lambda v: np.array([np.inf if x == "inf" else -np.inf if x == "-inf" else x for x in v], dtype=np.float64)
    base = dict(m=gold["m"], n=gold["n"], offsets=np.array(gold["offsets"], np.int32), indices=np.array(gold["indices"], np.int32),
                values=dec(gold["values"]), c=dec(gold["c"]), lo=dec(gold["lo"]), hi=dec(gold["hi"]), lb=dec(gold["lb"]), ub=dec(gold["ub"]),
                maximize=bool(gold["maximize"]), objective_offset=float(gold["objective_offset"]))
    integer = np.array([t == "I" for t in gold["var_types"]])
    m, n, nnz = base["m"], base["n"], int(len(base["values"]))
    rounds, limit = 6, 4000
    kw = dict(mode=1, device=local_rank, iteration_limit=limit)

    def make(count, share_stream):
        out = []
        for i in range(count):
            if share_stream and out:
                capi.lib.pdlpdev_create_share_stream(C.c_void_p(capi.lib.cuoptamd_solver_device(out[0].handle)))
            out.append(capi.Solver(base, **kw))
        capi.lib.pdlpdev_create_share_stream(None)
        return out

    def branch(l, lb, ub, x, rng):
        """the node's next child: an integer variable with a fractional relaxation value (a random integer one when all are integral);
        returns the variable (-1: none)"""
        frac = np.abs(x - np.round(x))
        cand = np.flatnonzero(integer & (frac > 1e-3) & (ub - lb >= 1.0))
        if len(cand) == 0:
            cand = np.flatnonzero(integer & (ub - lb >= 1.0))
        if len(cand) == 0:
            return -1
        j = int(rng.choice(cand))
        if l % 2 == 0:
            ub[j] = max(np.floor(x[j]), lb[j])
        else:
            lb[j] = min(np.ceil(x[j]), ub[j])
        return j

    def run(solvers, label, batch=None, executor=None):
        """the node sequence through `solvers`, same seeds and branches whoever solves.  batch: one cuoptamd_batch_branch per round (a
        variable and its new bounds per node, the start taken from the node's own last solution on the device), one
        cuoptamd_batch_advance, one cuoptamd_batch_solution_views.  executor: a worker of the pool takes a node through
        cuoptamd_solver_reset (full bounds + the solution read back), cuoptamd_solver_advance and cuoptamd_solver_get_solution.
        The choice of the branching variables is the caller's tree logic: timed, reported, not part of either rate."""
        rng = np.random.default_rng(17)
        k = len(solvers)
        lbs, ubs = [base["lb"].copy() for _ in range(k)], [base["ub"].copy() for _ in range(k)]
        t = dict(choose_branches=0.0, reset=0.0, advance=0.0, solution=0.0)
        its, statuses, objs = 0, {}, []
        prev = None
        for r in range(rounds + 1):  # round 0: the root relaxation in every node (cold)
            t0 = time.perf_counter()
            var = np.full(k, -1, np.int32)
            if r:
                for l in range(k):
                    var[l] = branch(l, lbs[l], ubs[l], prev[l][0], rng)
            t1 = time.perf_counter()
            if executor is not None:
                def node(l):
                    if r:
                        solvers[l].reset(lb=lbs[l], ub=ubs[l], init_x=prev[l][0], init_y=prev[l][1])
                    return solvers[l].advance(), solvers[l].solution()
                both = list(executor.map(node, range(k)))
                rs, prev = [q[0] for q in both], [q[1] for q in both]
                t2, t3 = t1, time.perf_counter()  # (the worker's reset + advance + read-back: all under "advance")
                t4 = t3
            else:
                if r:
                    jv = np.maximum(var, 0)
                    batch.branch(var, np.array([lbs[l][jv[l]] for l in range(k)]), np.array([ubs[l][jv[l]] for l in range(k)]))
                t2 = time.perf_counter()
                rs = batch.advance()
                t3 = time.perf_counter()
                prev = batch.solution_views()
                t4 = time.perf_counter()
            if r:  # the re-solves are what is measured
                t["choose_branches"] += t1 - t0
                t["reset"] += t2 - t1
                t["advance"] += t3 - t2
                t["solution"] += t4 - t3
                its += sum(q["steps_taken"] for q in rs)
                for q in rs:
                    statuses[q["status_name"]] = statuses.get(q["status_name"], 0) + 1
                objs.append([q["primal_objective"] for q in rs])
        total = t["reset"] + t["advance"] + t["solution"]
        return dict(label=label, lps=k * rounds, iterations=its, seconds={a: round(b, 4) for a, b in t.items()}, lps_per_sec=round(k * rounds / total, 1),
                    lps_per_sec_advance_only=round(k * rounds / t["advance"], 1), its_per_sec_advance=round(its / t["advance"], 1), statuses=statuses), objs, (lbs, ubs)

    def thread_pool_leg():
        kp = min(K, 64)
        pool_solvers = make(kp, False)
        ex = concurrent.futures.ThreadPoolExecutor(max_workers=16)
        run(pool_solvers, "warm-up", executor=ex)
        for s in pool_solvers:
            s.reset(lb=base["lb"], ub=base["ub"])
        pool, pobjs, _ = run(pool_solvers, "thread pool: 16 host threads over %d solvers (one stream each); a worker takes a node through reset, solve and read-back "
                             "(all three under 'advance')" % kp, executor=ex)
        ex.shutdown()
        for s in pool_solvers:
            s.close()
        same = all(a[:kp] == b for a, b in zip(objs, pobjs))
        return pool, same

    t0 = time.perf_counter()
    solvers = make(K, True)
    batch = capi.SmallBatch(solvers)
    create_s = time.perf_counter() - t0
    layout = solvers[0].device.layout()
    run(solvers, "warm-up", batch=batch)  # clocks, code objects, the allocator's pools
    batch.reset(lb=[base["lb"]] * K, ub=[base["ub"]] * K)
    got, objs, (lbs, ubs) = run(solvers, "small-LP batch: %d workgroups per launch; per round one cuoptamd_batch_branch, one cuoptamd_batch_advance, "
                                "one cuoptamd_batch_solution_views" % K, batch=batch)
    if args.dump_outputs:
        arrays = {}
        for l, (s, (x, y, z)) in enumerate(zip(solvers, batch.solutions())):
            arrays.update(solver_outputs(s.result.as_dict(), x, y, z, prefix="lp%04d_" % l))
        dump_outputs(args.dump_outputs, arrays)
    batch.close()
    for s in reversed(solvers):
        s.close()
    # ---- the same node sequences through a pool of host threads (one solver + one stream per LP; 16 threads)
    # (--no-convergence-run skips this leg: rocprofv3 7.2 crashes in a process that launches from sixteen threads)
    pool, same = None, None
    if args.full and not args.no_convergence_run:
        pool, same = thread_pool_leg()
    # ---- the reference's dual simplex (oracle/_ref, 1 thread) on a bounded sample of the LAST round's nodes (cold: it has no warm start here)
    cpu = None
    if args.full and not args.no_cpu_baseline:
        try:
            from oracle import refbind
            if refbind.available():
                t0, cnt = time.perf_counter(), 0
                for l in range(min(K, 24)):
                    refbind.dual_simplex(dict(base, lb=lbs[l], ub=ubs[l]), time_limit=20.0)
                    cnt += 1
                    if time.perf_counter() - t0 > 20.0:
                        break
                dt = time.perf_counter() - t0
                cpu = dict(value=round(cnt / dt, 2), unit="LP relaxations/s", cores=1, kind="reference",
                           sample="cpp/src/dual_simplex compiled in place (oracle/_ref), 1 thread, cold solves of %d nodes of the last round: %.2f s" % (cnt, dt))
        except Exception as e:
            cpu = dict(error=repr(e))
    info = capi.device_info(local_rank)
    bytes_iter = 24 * nnz + 4 * (m + n + 2) + 8 * (14 * n + 7 * m)
    eq = bytes_iter * got["its_per_sec_advance"] / 1e9
    out = {
        "metric": "pdlp_iterations_per_sec", "value": got["its_per_sec_advance"], "unit": "iterations/s (aggregate over %d LPs, inside the batch's advance calls)" % K,
        "lps_per_sec": got["lps_per_sec"], "lps_per_sec_unit": "warm-started re-solves to 1e-4 per second, whole pipeline (reset + advance + solution read-back)",
        "n_gpus": 1, "steps": args.steps, "warmup": args.warmup, "timed_steps": got["iterations"], "ms_per_step": round(1e3 * got["seconds"]["advance"] / max(got["iterations"], 1), 6),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "datasets/mip/50v-10-free-bound.mps (LP relaxation; tests/golden/problems.json)",
        "config": {"workload": "%s: %d branch-and-bound nodes of the 50v-10 LP relaxation (233 x 2013, 2745 nonzeros), %d rounds of one bound tightening per node + warm-started "
                               "re-solve to the default 1e-4 (iteration limit %d), Stable2 preset; persistent solvers, one small-LP batch" % (args.workload, K, rounds, limit),
                   "rows": m, "cols": n, "nnz": nnz, "lps": K, "rounds": rounds, "parallelism": "single GPU, %d LPs in %d workgroups per launch" % (K, K)},
        "batch": got, "thread_pool": pool, "batch_over_thread_pool_lps_per_sec": None if pool is None else round(got["lps_per_sec"] / pool["lps_per_sec"], 2),

        "same_objectives_as_the_thread_pool": same, "create_seconds_per_lp": round(create_s / K, 5),
        "roofline": dict(bound="hbm", kernel="k_pdhg_resident_batch", achieved=round(eq, 2), peak=HBM_PEAK_GBS, unit="GB/s", frac=round(eq / HBM_PEAK_GBS, 5), traffic=None,
                         note="the LP lives in registers and LDS of its workgroup: NOTHING is re-read from HBM inside the loop, so the HBM roofline does not bound this kernel -- "
                              "`achieved` is what a streaming implementation would have to move for the same iterations (fused floor %d B per iteration per LP); the loop is bound by "
                              "LDS / barrier latency: 5 barriers and ~13 dependent phases per attempt (DESIGN 4b)" % bytes_iter),
        "cpu_baseline": cpu, "spmv_layout": layout, "device": info["name"], "compute_units": info["compute_units"],
    }
    sys.stdout.flush()
    os.write(record_fd, (json.dumps(out) + "\n").encode())


def main():
    # stdout carries exactly ONE line, the JSON record: libraries loaded below write banners to file descriptor 1 (RCCL prints its
    # version block there when the first communicator is created), so everything else is sent to stderr
    sys.stdout.flush()
    record_fd = os.dup(1)
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--workload", default="c3", choices=["c3", "c2", "tiny", "hard", "banded", "staircase", "block_angular", "powerlaw", "multiband", "dense_rows", "c3x10", "banded4",
                             "banded_shuffled", "staircase_shuffled", "block_angular_shuffled", "multiband_shuffled", "c3x100", "c3x200", "c5_batch256", "c5_batch64", "c5_batch1024", "c3_batch16", "c3_batch8", "c3_batch4", "c3_batch2", "c2_batch16", "c2_batch8", "c2_batch4"],
                    help="*_shuffled: the structured family under a seeded random row AND column permutation (the set-up's analysis pass has to find the structure)")
    ap.add_argument("--min-seconds", type=float, default=0.0, help="lower bound on the duration of the timed region (timed_steps is rounded up "
                    "to whole major-iteration periods): long enough for an outside observer that samples the GPU every few seconds; 0 = exactly --steps")
    ap.add_argument("--full", action="store_true", help="also the legs beyond the headline figure: per-kernel times and roofline, the run to 1e-4, "
                    "the CPU baselines, the shader clock, the batch workloads' single-LP and thread-pool comparisons")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the timed path computed in its last step as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(with --full) leave out the CPU baselines")
    ap.add_argument("--no-convergence-run", action="store_true", help="(with --full) leave out the run to 1e-4 and the thread-pool leg")
    ap.add_argument("--force-comm", action="store_true", help="use the RCCL path even with one rank")
    ap.add_argument("--graph-comm", action="store_true", help="capture the collectives of a sharded attempt into the attempt graphs (pdlpdev_set_graph_mode 2)")
    ap.add_argument("--self-launch", action="store_true", help="go through the torch.distributed.run launcher also for one GPU")
    ap.add_argument("--spmv-layout", default=None, choices=["auto", "stream", "panel", "jag", "pb", "timed"], help="CUOPT_AMD_SPMV_LAYOUT")
    args = ap.parse_args()

    if args.spmv_layout:
        os.environ["CUOPT_AMD_SPMV_LAYOUT"] = args.spmv_layout
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" not in os.environ and (args.gpus > 1 or args.self_launch):
        # not under a launcher: start one process per GPU ourselves and relay rank 0's record
        import socket
        import subprocess
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        child = [a for a in sys.argv[1:] if a != "--self-launch"]
        if args.gpus == 1 and "--force-comm" not in child:
            child.append("--force-comm")
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + child
        r = subprocess.run(cmd, stdout=subprocess.PIPE, env=env)
        record = [ln for ln in r.stdout.decode(errors="replace").splitlines() if ln.startswith("{")]
        if record:
            os.write(record_fd, (record[-1] + "\n").encode())
        sys.exit(r.returncode if r.returncode else (0 if record else 1))
    if world != args.gpus:
        args.gpus = world
    dist = None
    if world > 1 or args.force_comm:
        # torch first (its bundled HIP/RCCL libraries get the sonames), then our library
        import torch
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29531")
        visible = torch.cuda.device_count()
        if visible < world:
            # (after the launcher ran: every rank sees the same count and leaves; nobody waits in a rendezvous)
            sys.exit("bench.py: %d GPUs requested, %d visible" % (world, visible))
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", rank=rank, world_size=world)
    from cuopt_amd import capi, synthetic

    def barrier():
        if dist is not None:
            import torch
            dist.barrier()
            torch.cuda.synchronize()

    def max_over_ranks(v):
        if dist is None:
            return v
        import torch
        t = torch.tensor([v], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    def fresh_comm_id():
        """an RCCL unique id bootstraps ONE communicator per rank, and the library destroys it with the last solver that
        uses it: every solver of this script gets its own id (rank 0 draws, everybody receives)"""
        if dist is None:
            return None
        import torch
        buf = torch.zeros(128, dtype=torch.uint8, device="cuda")
        if rank == 0:
            buf.copy_(torch.frombuffer(bytearray(capi.comm_unique_id()), dtype=torch.uint8))
        dist.broadcast(buf, 0)
        return bytes(buf.cpu().numpy().tobytes())

    comm_id = fresh_comm_id()

    if args.workload.startswith("c5_batch"):
        if world != 1:
            sys.exit("bench.py: the small-LP batch runs on one GPU")
        small_batch_line(args, int(args.workload[len("c5_batch"):]), local_rank, record_fd)
        return
    shuffle = args.workload.endswith("_shuffled")
    base = args.workload[:-len("_shuffled")] if shuffle else args.workload
    batch_k = int(base.split("_batch")[1]) if "_batch" in base else 0
    if batch_k:
        base = base.split("_batch")[0]
    structured = base in ("staircase", "block_angular", "powerlaw", "multiband", "dense_rows")
    if base == "hard":
        cfg = dict(synthetic.CONFIGS["c3"], hard=True)
    elif base == "banded4":
        cfg = dict(synthetic.CONFIGS["banded4"])
    elif structured:
        cfg = dict(kind=base, m=1_000_000, n=1_000_000, k=10, seed=7)
    elif base == "c3x100":
        cfg = dict(m=30_000_000, n=30_000_000, k=33, seed=2)
    elif base == "c3x200":  # 1.98e9 nonzeros: the "2 B nonzeros" the reference's FAQ names as its capacity (int32 offsets: < 2^31)
        cfg = dict(m=60_000_000, n=60_000_000, k=33, seed=2)
    else:
        cfg = dict(synthetic.CONFIGS[base])
    t_gen = time.time()
    # (profiling sessions run the same workload through several rocprofv3 passes: CUOPT_AMD_LP_CACHE=<dir> keeps the generated LP
    # between them -- the generator is deterministic, the cache only saves its minute of host time)
    cache = os.environ.get("CUOPT_AMD_LP_CACHE")
    cache_file = os.path.join(cache, "%s.npz" % (base if batch_k else args.workload)) if cache else None
    if cache_file and os.path.exists(cache_file):
        z = np.load(cache_file, allow_pickle=False)
        p = {k: (z[k] if z[k].ndim else z[k].item()) for k in z.files}
    elif args.workload in ("c3x100", "c3x200"):
        # 3e7 x 3e7 with 33 nonzeros per row: 9.9e8 nonzeros, generated ON THE DEVICE (pdlpdev_synthetic_lp: the host generator would
        # need minutes and tens of GB) -- the scale the reference's FAQ names for one 80 GB GPU (docs/cuopt/source/faq.rst:368-370)
        p = capi.synthetic_lp_on_device(cfg["m"], cfg["n"], cfg["k"], seed=cfg["seed"], device=local_rank)
        args.no_cpu_baseline = True  # (the oracle's loop at 1e9 nonzeros is minutes per iteration: no bounded sample fits the line's budget)
    else:
        p = synthetic.generate_structured(**cfg) if structured else synthetic.generate(**cfg)
        if shuffle:
            p = synthetic.shuffled(p, seed=5)
            p.pop("shuffle", None)
        if cache_file and rank == 0 and args.workload not in ("c3x100", "c3x200"):
            os.makedirs(cache, exist_ok=True)
            np.savez(cache_file, **{k: v for k, v in p.items() if isinstance(v, (np.ndarray, int, float, bool, np.integer, np.floating))})
    t_gen = time.time() - t_gen
    m, n, nnz = p["m"], p["n"], int(len(p["values"]))
    if batch_k:
        if world != 1:
            sys.exit("bench.py: the shared-matrix batch runs on one GPU")
        batch_line(args, p, cfg, batch_k, local_rank, record_fd, t_gen)
        return

    # ---- fixed-budget run: iterations / second ------------------------------------------------------
    # A PDLP iteration carries its amortised share of the major-iteration work (every `major_iteration` = 40 steps;
    # additionally EVERY step is a major iteration while the step count is <= min_iteration_restart, pdlp.cu:1082-1084).
    # Whatever --warmup says, the timed region therefore (i) starts past that initial phase, on a major-
    # iteration boundary, with every hipGraph replay size instantiated, and (ii) covers exactly --steps iterations (timed_steps;
    # --min-seconds lengthens it, (iv) below).  `steps` is reported as given, `timed_steps` and `warmup_done` as run; ms_per_step = elapsed / timed_steps.
    solver = capi.Solver(p, mode=1, tol=0.0, device=local_rank, rank=rank, world=world, comm_id=comm_id)
    setup_s = solver.advance(0)["setup_seconds"]
    dev = solver.device
    if args.graph_comm:
        dev.call("set_graph_mode", 2)
    dev.call("prepare_graphs")
    period = max(int(solver.hyper.major_iteration), 1)
    pre = max(args.warmup, 2 * period, int(solver.hyper.min_iteration_restart) + period)
    pre = ((pre + period - 1) // period) * period
    timed_steps = max(args.steps, 1)
    solver.advance(pre)
    layout = dev.layout()
    reorder = solver.reorder_info()
    dataflow = capi.lib.pdlpdev_shard_dataflow(dev.handle)  # read while the solver (and its device context) is alive
    transport = ", direct peer stores" if world > 1 and capi.lib.pdlpdev_shard_transport(dev.handle) == 1 else ""
    sharding = None
    if dist is not None:  # what a multi-rank line needs to be read without the code: ranks, dataflow, transport, halo, bytes on the wire
        wire = np.zeros(3, dtype=np.int64)
        capi.lib.pdlpdev_shard_wire_bytes(dev.handle, wire.ctypes.data_as(capi.C.c_void_p))
        sharding = dict(rccl_nranks=world,
                        dataflow={0: "none", 1: "all-reduce of the A^T y' partials (replicated primal)", 2: "reduce-scatter + all-gather (sliced primal)",
                                  3: "owner computes: all-gather(xbar slices) + all-gather(y' row blocks)"}.get(dataflow, str(dataflow)),
                        transport="direct peer stores into landing blocks + epoch flags (p2p)" if capi.lib.pdlpdev_shard_transport(dev.handle) == 1 else "RCCL collectives",
                        halo_exchange=bool(wire[0]), bytes_received_per_attempt_this_rank=int(wire[1] if wire[0] else wire[2]),
                        bytes_of_the_two_all_gathers=int(wire[2]),
                        collectives_in_graphs=bool(args.graph_comm))
    # ... and (iii) starts at the device's steady clocks: a GPU that sat idle while the LP was generated runs its first tens of
    # milliseconds below them (measured: the same 200 timed steps gave 4.7 k it/s right after start-up and 5.7 k once warm), so
    # untimed batches of five periods run until two consecutive batches agree within 2 % (at most 4 s).  Every rank takes the same
    # decision: the batch times are max-reduced over the ranks first.
    fixed_pre = pre
    warm_rates, warm_wall = [], 0.0
    while True:
        dev.call("synchronize")
        barrier()
        tb = time.perf_counter()
        solver.advance(5 * period)
        dev.call("synchronize")
        barrier()
        dt = max_over_ranks(time.perf_counter() - tb)
        pre += 5 * period
        warm_wall += dt
        warm_rates.append(5 * period / dt)
        steady = len(warm_rates) >= 3 and all(abs(warm_rates[-i] - warm_rates[-i - 1]) <= 0.02 * warm_rates[-i] for i in (1, 2))
        if steady or warm_wall > 4.0 or len(warm_rates) >= 100:
            break
    # ... and (v) the number of those batches depends on the clocks: the solver starts again from its fresh state (cuoptamd_solver_reset:
    # bit for bit a solver created anew) and runs a fixed warm-up (SETTLE_PERIODS), so that the timed steps -- and what --dump-outputs
    # writes -- are the same iterations in every run with the same arguments
    solver.reset()
    if args.graph_comm:  # (the reset went back to the settings' graph mode)
        dev.call("set_graph_mode", 2)
    dev.call("prepare_graphs")
    pre = fixed_pre + SETTLE_PERIODS * period
    solver.advance(pre)
    # (iv) with --min-seconds S > 0 the timed region lasts at least S seconds whatever --steps says, so that an outside observer
    # (rocm-smi samples, its own clock) sees the GPU leg: timed_steps is rounded up from the steady rate of the warm-up batches
    # (max-reduced over the ranks: same decision everywhere); `steps` is echoed as given, `timed_steps` as run.
    steady_rate = max_over_ranks(warm_rates[-1])
    if args.min_seconds > 0:
        timed_steps = max(timed_steps, int(np.ceil(args.min_seconds * steady_rate / period)) * period)
    dev.call("synchronize")
    barrier()
    # (the shader clock is sampled by a host thread WHILE the timed region runs: a reading taken in front of it would idle the GPU)
    import threading
    sclk_samples, sclk_stop = [], threading.Event()

    def sample_clock():
        while not sclk_stop.is_set():
            v = shader_clock_mhz()
            if v is not None:
                sclk_samples.append(v)
            sclk_stop.wait(0.4)
    sampler = threading.Thread(target=sample_clock, daemon=True) if rank == 0 and args.full else None
    if sampler:
        sampler.start()
    t0 = time.perf_counter()
    r = solver.advance(timed_steps)
    dev.call("synchronize")
    barrier()
    elapsed = max_over_ranks(time.perf_counter() - t0)
    sclk_stop.set()
    if sampler:
        sampler.join(timeout=30)
    steps_done = r["steps_taken"] - pre
    assert r["status"] == 0 and steps_done == timed_steps, (r["status_name"], steps_done)
    its_per_s = timed_steps / elapsed
    attempts = r["attempted_steps"]
    if rank == 0 and args.dump_outputs:
        x, y, z = solver.solution()
        dump_outputs(args.dump_outputs, solver_outputs(r, x, y, z))

    def emit(roofline, conv, cpu):
        if rank == 0:
            info = capi.device_info(local_rank)
            out = {
                "metric": "pdlp_iterations_per_sec", "value": round(its_per_s, 2), "unit": "iterations/s",
                "n_gpus": world, "rccl_nranks": world if dist is not None else 0, "steps": args.steps, "warmup": args.warmup, "timed_steps": timed_steps, "warmup_done": pre, "clock_warmup_batches": len(warm_rates),
                "ms_per_step": round(1e3 * elapsed / timed_steps, 5), "higher_is_better": True,
                "scaling": "strong", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
                "config": {"workload": "%s: synthetic %s sparse LP S(m=%d,n=%d,k=%d,seed=%d%s), nnz=%d, longest row %d, CSR fp64/int32, "
                                       "Stable2 preset, tolerances 0 (fixed iteration budget)"
                                       % (args.workload, ("structured (cuopt_amd/synthetic.py generate_structured)" if structured else "random") + (", rows and columns shuffled (synthetic.shuffled, seed 5)" if shuffle else ""),
                                          m, n, cfg["k"], cfg["seed"], (",hard" if cfg.get("hard") else "") + (",band=%d" % cfg["band"] if cfg.get("band") else ""),
                                          nnz, int(np.diff(p["offsets"]).max())),
                           "rows": m, "cols": n, "nnz": nnz,
                           "parallelism": ("row-block x%d + RCCL %s" % (world, {1: "all-reduce (replicated primal)", 2: "reduce-scatter / all-gather (sliced primal)",
                                                                           3: "owner computes: all-gather(xbar) + all-gather(y'), rows and columns of A per rank"}.get(dataflow, "?") + transport)) if world > 1 else "single GPU"},
                "roofline": roofline, "cpu_baseline": cpu, "time_to_1e-4": conv, "sharding": sharding,
                "spmv_layout": layout, "setup_reordering": reorder, "attempted_steps": attempts, "setup_seconds": round(setup_s, 4), "generate_seconds": round(t_gen, 2),
                "device": info["name"], "compute_units": info["compute_units"], "sclk_mhz_during_timed_region": {"samples": len(sclk_samples), "min": min(sclk_samples) if sclk_samples else None, "max": max(sclk_samples) if sclk_samples else None},
            }
            sys.stdout.flush()
            os.write(record_fd, (json.dumps(out) + "\n").encode())
        if dist is not None:
            dist.destroy_process_group()

    if not args.full:  # a plain run: the headline figure and nothing else
        solver.close()
        emit(None, None, None)
        return

    # ---- the attempt time the per-kernel times are held against (the guard below), from a run of its own over whole
    # major-iteration periods and at least 2 s: the timed region above may be a few steps long
    solver.advance((period - timed_steps % period) % period)
    dev.call("synchronize")
    barrier()
    guard_steps = max(5, int(np.ceil(2.0 * steady_rate / period))) * period
    guard_attempts_before = solver.advance(0)["attempted_steps"]
    t0 = time.perf_counter()
    rg = solver.advance(guard_steps)
    dev.call("synchronize")
    barrier()
    guard_elapsed = max_over_ranks(time.perf_counter() - t0)
    guard_attempts = rg["attempted_steps"] - guard_attempts_before  # rejected attempts cost a full set of kernels too

    # ---- per-kernel timing with HIP events on the solver stream (dominant kernel -> roofline) --------
    r0, r1 = solver.row_range()
    ml = r1 - r0
    nnz_l = int(p["offsets"][r1] - p["offsets"][r0])
    kernels = {}
    reps = 50 if nnz >= 5_000_000 else 200
    names = ["PRIMAL", "SPMV_A_DUAL", "SPMV_AT_STEP", "STEP_DECISION", "SPMV_A_PLAIN", "SPMV_AT_PLAIN"]
    for k in names:
        kernels[k] = dev.time_kernel(k, reps)
    bytes_alg = {
        # 12 B per nonzero + row offsets + every gathered vector entry once + the fused epilogue streams
        "SPMV_A_DUAL": 12 * nnz_l + 4 * (ml + 1) + 8 * n + 8 * (4 * ml + 2 * ml),   # y,lo,hi,sum_y r ; y',sum_y w
        "SPMV_AT_STEP": 12 * nnz_l + 4 * (n + 1) + 8 * ml + 8 * (3 * n + n),        # x,x',AtY r ; AtY' w
        "PRIMAL": 8 * (6 * n + 3 * n),                                            # x,c,AtY,lb,ub,sum_x r ; x',xbar,sum_x w
        "SPMV_A_PLAIN": synthetic.spmv_bytes(ml, n, nnz_l),
        "SPMV_AT_PLAIN": synthetic.spmv_bytes(n, ml, nnz_l),
    }
    dom = "SPMV_A_DUAL" if kernels["SPMV_A_DUAL"] >= kernels["SPMV_AT_STEP"] else "SPMV_AT_STEP"
    achieved = bytes_alg[dom] / (kernels[dom] * 1e-3) / 1e9
    lname = layout["A" if dom == "SPMV_A_DUAL" else "At"]["layout"]
    prefix = {"panel": "k_panel_", "jag": "k_jag_", "stream": "k_spmv_", "resident": "k_spmv_", "pb": "k_pb_"}[lname]
    kname = prefix + ("a_dual" if dom == "SPMV_A_DUAL" else "at_step")
    # HBM/fabric bytes per launch of that kernel from the committed rocprofv3 --pmc passes of this very
    # command (profiles/r03_pmc_<workload>.json, FETCH_SIZE x2 + WRITE_SIZE per MI355X_MICROARCH.md); the
    # counters cannot be read from inside the process, so this is null for workloads without a profile
    traffic, traffic_file = None, None
    for rnd in ("r06", "r05", "r04", "r03", "r02"):  # the newest committed PMC summary of this workload
        try:
            pmc = json.load(open(os.path.join(ROOT, "profiles", "%s_pmc_%s.json" % (rnd, args.workload))))
            if world == 1 and kname in pmc:
                traffic, traffic_file = round(pmc[kname]["traffic_bytes_corrected"]), "profiles/%s_pmc_%s.json" % (rnd, args.workload)
                break
        except Exception:
            pass
    roofline = dict(bound="hbm", kernel=kname,
                    achieved=round(achieved, 1), peak=HBM_PEAK_GBS, unit="GB/s",
                    frac=round(achieved / HBM_PEAK_GBS, 4), traffic=traffic,
                    algorithmic_bytes_per_launch=bytes_alg[dom], avg_launch_ms=round(kernels[dom], 5),
                    per_kernel_ms={k: round(v, 5) for k, v in kernels.items()},
                    per_kernel_gbs={k: round(bytes_alg[k] / (kernels[k] * 1e-3) / 1e9, 1) for k in bytes_alg},
                    iteration_fused_floor_bytes=synthetic.iteration_bytes_min(m, n, nnz),
                    iteration_frac_of_peak=round(synthetic.iteration_bytes_min(m, n, nnz) * its_per_s / 1e9
                                                 / HBM_PEAK_GBS / max(world, 1), 4),
                    traffic_calibrated=None if traffic is None else True,  # streams: MI355X_MICROARCH.md (FETCH_SIZE x 2); scattered 8-byte reads: profiles/r05_gather_calibration.txt (one 128-B line per miss, tallied at 64 B); WRITE_SIZE: k_primal 71.5 vs 72 MB
                    traffic_source=None if traffic is None else
                    "%s: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of `bench.py --workload %s` on the tree of round %s (scripts/gpu_session.sh pmc:%s; "
                    "2*FETCH+WRITE KiB, MI355X_MICROARCH.md HBM section) -- NOT measured by this run: counters cannot be read from inside the process%s"
                    % (traffic_file, args.workload, traffic_file.split("/")[1][1:3], args.workload, "" if traffic_file.startswith("profiles/r06") else "; an OLDER round's pass, kept because the kernel's timing has not moved since"))
    # Guard (round-3 review): the four kernels of an attempt, each timed on its own, must add up to the time of an attempt as the guard
    # run above saw it (the rest is the amortised major-iteration work and the graph's launch gaps).  A call site whose launches are not
    # all summed (a multi-launch layout timed as one phase), or a timed region that skipped work, shows up here.
    per_attempt_ms = 1e3 * guard_elapsed / max(guard_attempts, 1)
    ksum = sum(kernels[k] for k in ("PRIMAL", "SPMV_A_DUAL", "SPMV_AT_STEP", "STEP_DECISION"))
    roofline["attempt_kernels_ms"] = round(ksum, 5)
    roofline["ms_per_attempt"] = round(per_attempt_ms, 5)
    roofline["attempt_kernels_over_ms_per_attempt"] = round(ksum / per_attempt_ms, 4)
    if world == 1 and dist is None and args.workload == "c3":  # the headline line is refused outright; other lines carry the ratio
        assert 0.85 <= ksum / per_attempt_ms <= 1.05, \
            "per-kernel times (%.5f ms) do not add up to the attempt (%.5f ms): %r" % (ksum, per_attempt_ms, kernels)
    solver.close()

    # ---- run to the default 1e-4 termination: wall clock incl. setup -----------------------------------
    conv = None
    if not args.no_convergence_run:
        barrier()
        t0 = time.perf_counter()
        s2 = capi.Solver(p, mode=1, device=local_rank, rank=rank, world=world, comm_id=fresh_comm_id())
        rr = s2.advance()
        wall = max_over_ranks(time.perf_counter() - t0)
        conv = dict(status=rr["status_name"], iterations=rr["steps_taken"], wall_s=round(wall, 4),
                    setup_s=round(rr["setup_seconds"], 4), loop_s=round(rr["loop_seconds"], 4),
                    objective=rr["primal_objective"], objective_known=p["objective_star"],
                    relative_gap=rr["relative_gap"], rel_primal_residual=rr["l2_relative_primal_residual"],
                    rel_dual_residual=rr["l2_relative_dual_residual"], restarts=rr["num_restarts"])
        s2.close()

    # ---- CPU baseline: the C oracle's PDLP loop on the same LP, bounded iteration budget -----------------
    cpu = None
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline_block(p)

    emit(roofline, conv, cpu)


if __name__ == "__main__":
    main()
