"""Zero skip (CUOPT_AMD_TUNE=zero_skip) on the headline LP: how many entries of the gathered vectors are exactly 0.0 in the timed
range of bench.py, and what the bitmap costs the A product when none is -- the same LP with its lower bounds moved to -1.

    python scripts/zero_skip_probe.py [--steps 1200] [--reps 30]
    rocprofv3 ... -- python scripts/zero_skip_probe.py --profile [--steps 2400]

Without --profile: one JSON line per (bounds, zero_skip) pair, each pair twice: zero fractions of XBAR and of the dual iterate behind
`steps` iterations, the control block's flag, and pdlpdev_time_kernel's average of the four kernels of an attempt (whole attempts in
the loop's order, the dispatch's own timestamps).  zero_skip=1 on the shifted LP is the guard's "off" state: bitmap written, flag down.
--profile: `steps` iterations of the headline LP with PLAIN launches (no graph replay: the profiler's interception of hipGraphLaunch is
what fell over under bench.py) and whatever CUOPT_AMD_TUNE the caller set -- the program to put behind rocprofv3 --kernel-trace --stats
or --pmc.  CUOPT_AMD_ROOT: the tree whose cuopt_amd package is measured (default: this script's)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.environ.get("CUOPT_AMD_ROOT", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=1200)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    from cuopt_amd import capi, synthetic
    p = synthetic.generate(**synthetic.CONFIGS["c3"])
    if args.profile:
        solver = capi.Solver(p, mode=1, tol=0.0)
        solver.device.call("set_graph_mode", 0)
        solver.advance(args.steps)
        print(json.dumps(dict(steps=int(solver.device.ctl().steps_taken), slabs_A=solver.device.layout()["A"]["slabs"])), flush=True)
        solver.close()
        return
    shifted = dict(p, lb=np.full(p["n"], -1.0))
    for bounds, q in (("lb=0", p), ("lb=-1", shifted)):
        for zs in (0, 1, 2, 0, 1, 2):
            os.environ["CUOPT_AMD_TUNE"] = "zero_skip=%d" % zs
            solver = capi.Solver(q, mode=1, tol=0.0)
            solver.advance(args.steps)
            dev = solver.device
            xbar, y, c = dev.download("XBAR", q["n"]), dev.download("Y", q["m"]), dev.ctl()
            out = dict(bounds=bounds, zero_skip=zs, steps=int(c.steps_taken), flag=int(getattr(c, "zskip", 0)), slabs_A=dev.layout()["A"]["slabs"],
                       xbar_zero_fraction=float(np.mean(xbar == 0.0)), y_zero_fraction=float(np.mean(y == 0.0)),
                       a_dual_us=1e3 * dev.time_kernel("SPMV_A_DUAL", args.reps), at_step_us=1e3 * dev.time_kernel("SPMV_AT_STEP", args.reps),
                       primal_us=1e3 * dev.time_kernel("PRIMAL", args.reps), decision_us=1e3 * dev.time_kernel("STEP_DECISION", args.reps))
            print(json.dumps(out), flush=True)
            solver.close()


if __name__ == "__main__":
    main()
