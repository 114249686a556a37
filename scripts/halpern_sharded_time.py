#!/usr/bin/env python3
"""Step cost of the sharded reflected-Halpern mode (cuoptamd_settings::halpern_sharded) at ONE rank behind a real communicator, beside
the attempt cost of a sharded Stable2 solver on the same LP, in the same build and session: one JSON line per run into --out, which a
run replaces (default profiles/halpern_sharded_time.jsonl), and a summary line per transport.  GPU only.

  python scripts/halpern_sharded_time.py [--workload c3|c2] [--runs 5] [--steps 400] [--transports collective,p2p] [--what run|advance] [--out FILE]

Per transport two solvers are created (mode 4 with halpern_sharded, mode 1; rank 0 of world 1, owner-computes dataflow) and advanced
alternately, `runs` times `steps` iterations each behind one warm-up advance; a run's figure is wall time over the steps (mode 4) or
over the attempts (mode 1) it made.  --what run (default): pdlpdev_run on the solver's device context -- the steps / attempts and
run_epilogue alone, no major iteration, so that steps are compared with attempts; --what advance: cuoptamd_solver_advance, major
iterations (evaluations, restarts) included.  Reported: the medians, the spread (max - min over the median) and the ratio of the medians."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WORKLOADS = {"c3": dict(m=1000000, n=1000000, k=10, seed=2), "c2": dict(m=100000, n=100000, k=10, seed=1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c3", choices=sorted(WORKLOADS))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--transports", default="collective,p2p")
    ap.add_argument("--what", default="run", choices=["run", "advance"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "halpern_sharded_time.jsonl"))
    args = ap.parse_args()
    lines = []
    for transport in args.transports.split(","):
        os.environ["CUOPT_AMD_SHARD_TRANSPORT"] = transport
        from cuopt_amd import capi, synthetic
        w = WORKLOADS[args.workload]
        p = synthetic.generate(w["m"], w["n"], w["k"], seed=w["seed"])
        solvers = {"halpern": capi.Solver(p, mode=4, halpern_sharded=1, tol=0.0, rank=0, world=1, comm_id=capi.comm_unique_id()),
                   "stable2": capi.Solver(p, mode=1, tol=0.0, rank=0, world=1, comm_id=capi.comm_unique_id())}
        done = {k: s.advance(args.steps) for k, s in solvers.items()}  # (warm-up: the first step as plain launches, the graphs captured)
        per = {k: [] for k in solvers}
        for run in range(args.runs):
            for k, s in solvers.items():
                if args.what == "run":
                    c0 = s.device.ctl()
                    t0 = time.perf_counter()
                    c = s.device.run(c0.steps_taken + args.steps)
                    dt = time.perf_counter() - t0
                    count = (c.steps_taken - c0.steps_taken) if k == "halpern" else (c.attempts - c0.attempts)
                else:
                    t0 = time.perf_counter()
                    r = s.advance(args.steps)
                    dt = time.perf_counter() - t0
                    count = (r["steps_taken"] - done[k]["steps_taken"]) if k == "halpern" else (r["attempted_steps"] - done[k]["attempted_steps"])
                    done[k] = dict(r)
                per[k].append(1e6 * dt / max(count, 1))
                lines.append(dict(workload=args.workload, transport=transport, what=args.what, solver=k, run=run, counted=count, us_each=per[k][-1]))
        for s in solvers.values():
            s.close()
        med = {k: statistics.median(v) for k, v in per.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in per.items()}
        summary = dict(workload=args.workload, transport=transport, what=args.what, summary=True, halpern_us_per_step=med["halpern"], stable2_us_per_attempt=med["stable2"],
                       halpern_spread=spread["halpern"], stable2_spread=spread["stable2"], ratio=med["halpern"] / med["stable2"])
        lines.append(summary)
        print(json.dumps(summary), flush=True)
    with open(args.out, "w") as f:
        for line in lines:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
