#!/usr/bin/env python
"""Where the microseconds of one major-iteration period go, out of a `rocprofv3 --kernel-trace --memory-copy-trace
--output-format csv` run of `bench.py --workload <w> --steps K` (no counters in that run).

  usage: period_budget.py <trace dir> [--periods N] [--stats-csv FILE] [> profiles/...txt]

--stats-csv FILE: the per-kernel statistics of those periods in the columns of `rocprofv3 --stats` (Name, Calls, TotalDurationNs,
AverageNs, Percentage, MinNs, MaxNs, StdDev), for a like-for-like comparison of two builds over the same iterations.

The timed region is the tail of the trace (a plain bench run closes the solver right behind it), and every period starts with the
one k_set_target of the call that runs its attempts and ends with its major iteration, so the trace is cut in front of every
k_set_target and the last N periods are kept (default 10 = --steps 400 at a period of 40).  Per period, on
average: the attempt kernels, the evaluation products, the other kernels, the copies (the runtime performs a small D2H copy
either as a DMA copy, which shows in the memory-copy trace, or as its blit kernel __amd_rocclr_copyBuffer, which shows in the
kernel trace: both are counted as copies), and the IDLE time of the queue: every gap between the end of one dispatch or copy
and the start of the next, split into the gaps that follow a copy (a host round trip: copy, synchronise, decide, enqueue),
the gaps between two attempt kernels (inside the replay of the attempt graphs: under the tracer a replay of 32 + 8 attempts
stalls for milliseconds where the untraced run does not -- an artefact of the tool, listed so that it is not mistaken for
the period's own idle time) and all others (launch-to-launch dependencies around the major iteration)."""
import argparse
import collections
import csv
import glob
import os
import re

ATTEMPT = re.compile(r"k_(panel|jag|stream|pb|gf)?_?(a_dual|at_step)|k_primal\b|k_step_decision\b|k_dense_")
EVAL = re.compile(r"k_(panel_|jag_|stream_|pb_|gf_)?eval_(dual|primal)(?!_from|_elementwise)")
TWIN = re.compile(r"eval_dual_from_aty")
COPY_KERNEL = re.compile(r"__amd_rocclr_copyBuffer")


def short(name):
    name = name.split("(")[0]
    return re.sub(r"^void ", "", re.sub(r"\(anonymous namespace\)::", "", name))


def load(trace_dir):
    ev = []  # (start, end, kind, name)
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            name = short(r["Kernel_Name"])
            kind = "copy" if COPY_KERNEL.search(name) else "kernel"
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), kind, name))
    for f in glob.glob(os.path.join(trace_dir, "**", "*memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), "copy", "copy " + r.get("Direction", "?")))
    ev.sort()
    return ev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace_dir")
    ap.add_argument("--periods", type=int, default=10)
    ap.add_argument("--stats-csv", default=None)
    a = ap.parse_args()
    ev = load(a.trace_dir)
    if not ev:
        raise SystemExit("no *kernel_trace.csv under %s" % a.trace_dir)
    # every call that runs a period's attempts starts with exactly one k_set_target (make-up rounds for rejected attempts stay inside
    # the call), and the major iteration that ends the period comes before the next one
    starts = [i for i, e in enumerate(ev) if e[2] == "kernel" and "k_set_target" in e[3]]
    # the tail: the last period ends with the last major iteration's last kernel or copy
    starts.append(len(ev))
    if len(starts) - 1 < a.periods:
        raise SystemExit("only %d periods in the trace" % (len(starts) - 1))
    cuts = starts[-(a.periods + 1):]
    n = a.periods
    per_kernel = collections.defaultdict(lambda: [0, 0])
    durations = collections.defaultdict(list)
    cls = collections.defaultdict(lambda: [0, 0])
    gaps = {"after a copy": [0, 0], "between attempt kernels (tracer)": [0, 0], "other": [0, 0]}
    wall = 0
    big = []
    for p in range(n):
        seg = ev[cuts[p]:cuts[p + 1]]
        # (the gap in front of the next period's first event belongs to this period: the host decides there)
        nxt = ev[cuts[p + 1]][0] if cuts[p + 1] < len(ev) else seg[-1][1]
        wall += nxt - seg[0][0]
        for k, (s, e, kind, name) in enumerate(seg):
            per_kernel[name][0] += 1
            per_kernel[name][1] += e - s
            durations[name].append(e - s)
            c = ("copies" if kind == "copy" else "attempt kernels" if ATTEMPT.search(name) else "evaluation products" if EVAL.search(name)
                 else "evaluation twin (no product)" if TWIN.search(name) else "other kernels")
            cls[c][0] += 1
            cls[c][1] += e - s
            following = seg[k + 1][0] if k + 1 < len(seg) else nxt
            nxt_attempt = k + 1 < len(seg) and seg[k + 1][2] == "kernel" and ATTEMPT.search(seg[k + 1][3])
            g = following - e
            if g > 0:
                w = gaps["after a copy" if kind == "copy" else "between attempt kernels (tracer)" if (c == "attempt kernels" and nxt_attempt) else "other"]
                w[0] += 1
                w[1] += g
                if g > 20000:
                    big.append((g, name))
    print("period budget: %d periods at the tail of the trace, %d dispatches and copies; per period on average" % (n, cuts[-1] - cuts[0]))
    print("%-44s %10s %12s" % ("", "count", "us"))
    busy = 0
    for c in ("attempt kernels", "evaluation products", "evaluation twin (no product)", "other kernels", "copies"):
        print("%-44s %10.1f %12.1f" % (c, cls[c][0] / n, cls[c][1] / n / 1e3))
        busy += cls[c][1]
    for c in ("after a copy", "between attempt kernels (tracer)", "other"):
        print("%-44s %10.1f %12.1f" % ("idle: gaps " + c, gaps[c][0] / n, gaps[c][1] / n / 1e3))
    print("%-44s %10s %12.1f" % ("period, first start to next period's start", "", wall / n / 1e3))
    print("%-44s %10s %12.1f" % ("  of it busy", "", busy / n / 1e3))
    tracer = gaps["between attempt kernels (tracer)"][1]
    print("%-44s %10s %12.1f" % ("  without the gaps between attempt kernels", "", (wall - tracer) / n / 1e3))
    print()
    print("gaps above 20 us: %d in all%s" % (len(big), "".join("\n  %.1f us behind %s" % (g / 1e3, nm) for g, nm in sorted(big, reverse=True)[:12])))
    print()
    print("%-44s %10s %12s %12s" % ("kernel / copy", "per period", "us each", "us / period"))
    for name, (cnt, tot) in sorted(per_kernel.items(), key=lambda kv: -kv[1][1]):
        print("%-44s %10.2f %12.2f %12.1f" % (name[-44:], cnt / n, tot / cnt / 1e3, tot / n / 1e3))
    if a.stats_csv:
        total = sum(sum(d) for d in durations.values()) or 1
        with open(a.stats_csv, "w", newline="") as f:
            w = csv.writer(f, quoting=csv.QUOTE_NONNUMERIC)
            w.writerow(["Name", "Calls", "TotalDurationNs", "AverageNs", "Percentage", "MinNs", "MaxNs", "StdDev"])
            for name, d in sorted(durations.items(), key=lambda kv: -sum(kv[1])):
                mean = sum(d) / len(d)
                sd = (sum((x - mean) ** 2 for x in d) / (len(d) - 1)) ** 0.5 if len(d) > 1 else 0.0
                w.writerow([name, len(d), sum(d), round(mean, 6), round(100.0 * sum(d) / total, 4), min(d), max(d), round(sd, 6)])


if __name__ == "__main__":
    main()
