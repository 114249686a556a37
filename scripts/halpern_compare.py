#!/usr/bin/env python3
"""Measurements of the restarted reflected-Halpern mode (solver mode 4) against Stable2 -> profiles/r09_halpern.jsonl.

  python scripts/halpern_compare.py [--out FILE] [--only cost|convergence|small] [--workloads c3,c2,...] [--parent-lib libcuopt.so]
                                    [--device-major 0,1,4,8]

* cost of a step: ms per step in mode 4 against ms per ATTEMPT of Stable2 (solves to a fixed iteration count from a warmed
  solver: wall time over attempted steps, five alternating runs each), plus the per-kernel durations of both modes from
  pdlpdev_time_kernel.  --parent-lib runs the Stable2 leg on another build of the library (a child process per leg: one process
  holds one library), which is how the step of this tree is compared with the attempt of the commit before it.
* iterations and wall time to 1e-4 and to 1e-8, mode 4 against Stable2 of the same build, on the synthetic families and the
  golden LPs with more than 50 rows.  Reported whichever way they fall; Stable2 stays the default preset.
* --only small (not part of the default run): the golden LPs of resident size at 1e-4 and 1e-8 in three variants -- mode 4 in the
  resident one-workgroup loop (halpern_resident = 1), mode 4 on the multi-launch path (--parent-lib: on that build, which is how the
  commit before the setting is measured), Stable2 -- five alternating rounds, one child process per variant and round; a record
  per LP and tolerance with all runs, their median and their spread (min, max), plus steps/s of the three loops over 4000
  steps of 50v-10 at tol = 0, likewise.  --device-major 0,1,4,8 adds, per P of the list, the resident loop with
  cuoptamd_settings::halpern_device_major = P (verdict and restart decided on the device, P periods per synchronisation; P = 0 runs
  on --parent-lib when one is given: the commit before the setting), with the synchronisations of the loop (pdlpdev_loop_stats)
  and the burst counters (pdlpdev_halpern_burst_stats: periods enqueued behind a stop are empty launches) in every record.
Every record is one JSON line: {"kind": "cost" | "kernels" | "convergence" | "small" | "small_rate", ...}; --out is written anew by every run.

Each leg is a child process of its own under a time limit sized to the leg.  The first leg that fails, is killed by a signal or
runs out of its time ends the whole run with a non-zero exit: nothing more is started on a GPU that has just shown trouble."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def problem(name):
    import numpy as np
    from cuopt_amd import synthetic
    if name in synthetic.CONFIGS:
        return synthetic.generate(**synthetic.CONFIGS[name])
    if name == "hard":
        return synthetic.generate(**dict(synthetic.CONFIGS["c3"], hard=True))
    if name in ("staircase", "block_angular"):
        return synthetic.generate_structured(name, m=1_000_000, n=1_000_000, k=10, seed=7)
    raw = json.load(open(os.path.join(ROOT, "tests", "golden", "problems.json")))[name]
    dec = lambda v: np.array([np.inf if x == "inf" else -np.inf if x == "-inf" else x for x in v], dtype=np.float64)
    return dict(m=raw["m"], n=raw["n"], offsets=np.array(raw["offsets"], np.int32), indices=np.array(raw["indices"], np.int32),
                values=dec(raw["values"]), c=dec(raw["c"]), lo=dec(raw["lo"]), hi=dec(raw["hi"]), lb=dec(raw["lb"]), ub=dec(raw["ub"]),
                maximize=bool(raw["maximize"]), objective_offset=float(raw["objective_offset"]))


def cost_leg(name, mode, steps, runs):
    """ms per attempted step of `mode`, `runs` times: a solver advanced by `steps` iterations after a warm-up of 200"""
    from cuopt_amd import capi
    p = problem(name)
    out = []
    for _ in range(runs):
        s = capi.Solver(p, mode=mode, tol=1e-30)
        s.advance(200)
        before = s.result.attempted_steps
        t0 = time.perf_counter()
        r = s.advance(steps)
        dt = time.perf_counter() - t0
        out.append(1e3 * dt / max(1, r["attempted_steps"] - before))
        if mode == 4 or len(out) == runs:
            kernels = {k: s.device.time_kernel(k, reps=20) for k in ("PRIMAL", "SPMV_A_DUAL", "SPMV_AT_STEP", "STEP_DECISION")}
        s.close()
    return dict(ms_per_step=out, kernels_ms=kernels)


def convergence_leg(name, mode, tol, limit):
    from cuopt_amd import capi
    p = problem(name)
    s = capi.Solver(p, mode=mode, tol=tol, iteration_limit=limit)
    r = s.advance()
    lay = s.device.layout()
    s.close()
    return dict(status=r["status_name"], iterations=r["steps_taken"], attempts=r["attempted_steps"], restarts=r["num_restarts"],
                loop_seconds=r["loop_seconds"], setup_seconds=r["setup_seconds"], objective=r["primal_objective"],
                layout=[lay["A"]["layout"], lay["At"]["layout"]])


SMALL = ["afiro", "mip-50v-10-free-bound-relaxation", "mip-neos5-free-bound-relaxation", "mip-sudoku-relaxation"]


def small_leg(names, mode, resident, limit, device_major=0):
    """every LP of `names` at 1e-4 and 1e-8 in one process (a warm-up solve of the first LP in front), then the loop's rate on 50v-10"""
    from cuopt_amd import capi
    kw = dict(halpern_resident=1) if resident else {}
    if device_major:
        kw["halpern_device_major"] = device_major
    out = {}
    for i, name in enumerate([names[0]] + names):
        p = problem(name)
        for tol in (1e-4, 1e-8):
            s = capi.Solver(p, mode=mode, tol=tol, iteration_limit=limit, **kw)
            r = s.advance()
            out["%s@%g" % (name, tol)] = dict(status=r["status_name"], iterations=r["steps_taken"], restarts=r["num_restarts"], loop_seconds=r["loop_seconds"],
                                               resident=bool(s.device.layout()["resident"]), majors=r["num_major_iterations"],
                                               loop_syncs=s.device.loop_stats()["loop_syncs"],
                                               burst=s.device.halpern_burst_stats() if device_major else None)
            s.close()
    s = capi.Solver(problem(SMALL[1]), mode=mode, tol=0.0, **kw)
    s.advance(400)
    t0 = time.perf_counter()
    s.advance(4000)
    s.device.call("synchronize")
    out["rate"] = 4000 / (time.perf_counter() - t0)
    s.close()
    return out


def summary(values):
    v = sorted(values)
    return dict(runs=values, median=v[len(v) // 2], min=v[0], max=v[-1])


def child(args):
    leg = json.loads(args.child)
    if leg["kind"] == "small":
        print(json.dumps(small_leg(leg["workloads"], leg["mode"], leg["resident"], leg["limit"], leg.get("device_major", 0))))
    elif leg["kind"] == "cost":
        print(json.dumps(cost_leg(leg["workload"], leg["mode"], leg["steps"], leg["runs"])))
    else:
        print(json.dumps(convergence_leg(leg["workload"], leg["mode"], leg["tol"], leg["limit"])))


def leg_seconds(leg):
    """time limit of a leg: the LP's generation and set-up (a minute at 1e7 nonzeros on a slow host) plus the steps it may take at a
    pessimistic millisecond each"""
    if leg["kind"] == "small":
        return 240
    steps = leg["steps"] + 200 if leg["kind"] == "cost" else leg["limit"]
    return 90 + steps // 1000


def run_child(leg, lib=None):
    env = dict(os.environ)
    if lib:
        env["CUOPT_AMD_LIB"] = os.path.abspath(lib)
    try:
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(leg)], env=env, capture_output=True, text=True,
                             timeout=leg_seconds(leg))
    except subprocess.TimeoutExpired:
        sys.exit("halpern_compare: leg %s ran out of its %d s: stopping, nothing more is started on this GPU" % (leg, leg_seconds(leg)))
    if out.returncode != 0:
        sys.exit("halpern_compare: leg %s ended with status %d: stopping, nothing more is started on this GPU\n%s" % (leg, out.returncode, out.stderr[-2000:]))
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_halpern.jsonl"))
    ap.add_argument("--only", default=None, choices=["cost", "convergence", "small"])
    ap.add_argument("--workloads", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--steps", type=int, default=6000)
    ap.add_argument("--limit", type=int, default=200000)
    ap.add_argument("--device-major", default=None, help="comma-separated P of halpern_device_major for --only small, e.g. 0,1,4,8")
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args)
    open(args.out, "w").close()

    def emit(rec):
        print(json.dumps(rec), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(rec) + "\n")

    if args.only in (None, "cost"):
        for w in (args.workloads.split(",") if args.workloads else ["c3", "c2", "banded"]):
            stable, halpern = [], []
            steps = args.steps * (20 if w == "c2" else 1)  # (c2: 0.03 ms per step -- a timed window of a second, like the others')
            for _ in range(5):  # alternating: the two legs see the same machine state
                a = run_child(dict(kind="cost", workload=w, mode=1, steps=steps, runs=1), lib=args.parent_lib)
                b = run_child(dict(kind="cost", workload=w, mode=4, steps=steps, runs=1))
                stable += a["ms_per_step"]
                halpern += b["ms_per_step"]
            emit(dict(kind="cost", workload=w, steps=steps, stable2_library="parent" if args.parent_lib else "this build", stable2_ms_per_attempt=stable,
                      halpern_ms_per_step=halpern, ratio_of_medians=sorted(halpern)[2] / sorted(stable)[2]))
            emit(dict(kind="kernels", workload=w, stable2_ms=a["kernels_ms"], halpern_ms=b["kernels_ms"]))
    if args.only == "small":
        names = args.workloads.split(",") if args.workloads else SMALL
        variants = (("halpern_resident", 4, True, None, 0), ("halpern_multi_launch", 4, False, args.parent_lib, 0), ("stable2", 1, False, None, 0))
        if args.device_major:  # the resident loop alone, per P (P = 0: the host-decided loop, on the parent's build when one is given)
            variants = tuple(("halpern_resident_P%d" % P, 4, True, args.parent_lib if P == 0 else None, P) for P in (int(v) for v in args.device_major.split(",")))
        runs = {v[0]: [] for v in variants}
        for _ in range(5):  # alternating: the variants see the same machine state
            for key, mode, resident, lib, major in variants:
                runs[key].append(run_child(dict(kind="small", workloads=names, mode=mode, resident=resident, limit=args.limit, device_major=major), lib=lib))
        for w in names:
            for tol in (1e-4, 1e-8):
                rec = dict(kind="small", workload=w, tol=tol, multi_launch_library="parent" if args.parent_lib else "this build")
                for key in runs:
                    legs = [r["%s@%g" % (w, tol)] for r in runs[key]]
                    rec[key] = dict(status=legs[0]["status"], iterations=legs[0]["iterations"], restarts=legs[0]["restarts"], resident=legs[0]["resident"],
                                    same_iterations_in_every_run=len({l["iterations"] for l in legs}) == 1, loop_seconds=summary([l["loop_seconds"] for l in legs]),
                                    majors=legs[0].get("majors"), loop_syncs=legs[0].get("loop_syncs"), burst=legs[0].get("burst"))
                emit(rec)
        emit(dict(kind="small_rate", workload=SMALL[1], steps=4000, steps_per_second={key: summary([r["rate"] for r in runs[key]]) for key in runs}))
    if args.only in (None, "convergence"):
        names = args.workloads.split(",") if args.workloads else ["c3", "c2", "hard", "banded", "staircase", "block_angular", "afiro",
                                                                  "mip-50v-10-free-bound-relaxation", "mip-neos5-free-bound-relaxation",
                                                                  "mip-sudoku-relaxation", "mip-cod105_max-relaxation"]
        for w in names:
            for tol in (1e-4, 1e-8):
                rec = dict(kind="convergence", workload=w, tol=tol)
                for mode, key in ((1, "stable2"), (4, "halpern")):
                    rec[key] = run_child(dict(kind="convergence", workload=w, mode=mode, tol=tol, limit=args.limit))
                emit(rec)


if __name__ == "__main__":
    main()
