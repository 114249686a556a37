#!/usr/bin/env python3
"""What infeasibility detection costs the reflected-Halpern mode (cuoptamd_settings::halpern_infeasibility;
docs/design/04d_halpern_mode.md, "Infeasibility detection") -> one JSON line per (workload, configuration), printed and written
to --out, which a run replaces (default profiles/halpern_infeasibility.jsonl).  GPU only.

  python scripts/halpern_infeasibility_time.py [--workloads c3,c2] [--runs 5] [--parent-lib libcuopt.so] [--out FILE]

bench.py has no switch for the solver mode, so the figure is the one of docs/design/07_measurement.md, "Halpern mode": ms per step
of mode 4 -- wall time of Solver.advance over a fixed step budget (c3: 6000 steps, c2: 120000; major iterations included) behind a
warm-up of 200 steps, tol = 1e-30 so that nothing ends the solve.  Configurations: the option off, the option on (the ray pass
behind every evaluation: two plain products per 40 steps), and with --parent-lib the same solve on another build of the library
(the commit before the option).  `runs` alternating rounds; every measurement is a child process of its own (one process holds one
library) under a time limit.  The first child that fails, is killed by a signal or runs out of its time ends the whole run with a
non-zero exit: nothing more is started on a GPU that has just shown trouble."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = {"c3": 6000, "c2": 120000}


def leg(name, on, steps):
    from cuopt_amd import capi, synthetic
    p = synthetic.generate(**synthetic.CONFIGS[name])
    kw = dict(halpern_infeasibility=1) if on else {}
    s = capi.Solver(p, mode=4, tol=1e-30, **kw)
    s.advance(200)
    before = s.result.attempted_steps
    t0 = time.perf_counter()
    r = s.advance(steps)
    dt = time.perf_counter() - t0
    lay = s.device.layout()
    out = dict(ms_per_step=1e3 * dt / max(1, r["attempted_steps"] - before), steps=r["attempted_steps"] - before, status=r["status_name"],
               major_iterations=r["num_major_iterations"], loop_syncs=s.device.loop_stats()["loop_syncs"],
               layout=[lay["A"]["layout"], lay["At"]["layout"]])
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c2")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "halpern_infeasibility.jsonl"))
    ap.add_argument("--leg", nargs=2, default=None, help=argparse.SUPPRESS)  # (a child: workload, 0 | 1)
    args = ap.parse_args()
    if args.leg:
        print("LEG " + json.dumps(leg(args.leg[0], args.leg[1] == "1", STEPS[args.leg[0]])), flush=True)
        return 0
    configs = ([("parent", 0, args.parent_lib)] if args.parent_lib else []) + [("off", 0, None), ("on", 1, None)]
    lines = []
    for name in args.workloads.split(","):
        runs = {c[0]: [] for c in configs}
        for _ in range(args.runs):
            for what, on, lib in configs:
                env = dict(os.environ)
                if lib:
                    env["CUOPT_AMD_LIB"] = os.path.abspath(lib)
                child = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name, str(on)], env=env, capture_output=True, text=True,
                                       timeout=240)
                got = [l for l in child.stdout.splitlines() if l.startswith("LEG ")]
                if child.returncode != 0 or not got:
                    sys.stderr.write(child.stdout + child.stderr)
                    sys.exit("%s / %s: the child ended with status %d" % (name, what, child.returncode))
                runs[what].append(json.loads(got[0][4:]))
        for what, _, _ in configs:
            ms = sorted(r["ms_per_step"] for r in runs[what])
            rec = dict(kind="halpern_infeasibility_cost", workload=name, configuration=what, steps=STEPS[name], ms_per_step=[r["ms_per_step"] for r in runs[what]],
                       median=ms[len(ms) // 2], min=ms[0], max=ms[-1], layout=runs[what][0]["layout"], loop_syncs=runs[what][0]["loop_syncs"],
                       major_iterations=runs[what][0]["major_iterations"])
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for rec in lines:
            f.write(json.dumps(rec) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
