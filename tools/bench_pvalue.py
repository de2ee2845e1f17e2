#!/usr/bin/env python3
"""Times the exact p-value thresholds (tfbs_patterns_pvalue_thresholds) of a C3-shaped set:
600 synthetic PWMs (tfbs_synth_write_pwms, length config 3, seed 3) on both strands.

By a host clock around the calls, as medians of --steps calls after --warmup, in one process
that should have the machine to itself:

  * device_ms: the call on HIP device --device (score_dist.hip; uploads, launches, the
    allocations of every scratch chunk and the copy-back included);
  * host_ms: the host twin (device = -1) on --threads host threads (TFBS_HOST_THREADS).

The two results must be equal.  As a recorded observation it also counts the strands whose exact
threshold differs from the one the generator's .thr table gives at the same p-value: that
table comes from a dynamic programme in double and is the thing compared, not the yardstick.
Prints one JSON line.

  python tools/bench_pvalue.py [--steps 5] [--warmup 1] [--pwms 600] [--pvalue 0.0001] [--threads 16]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, warmup):
    out, ms = None, []
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        out = fn()
        if i >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pwms", type=int, default=600)
    ap.add_argument("--pvalue", type=float, default=1e-4)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--skip_host", action="store_true")
    a = ap.parse_args()
    os.environ["TFBS_HOST_THREADS"] = str(a.threads)
    import tfbs_pkg

    T = tfbs_pkg.load()
    work = tempfile.mkdtemp(prefix="tfbs_bench_pvalue_")
    names = T.synth_write_pwms(work, a.pwms, 3, 3)
    ps = T.parse_pwm_files(os.path.join(work, "pwms.txt"), os.path.join(work, "thr"), a.pvalue, names)
    pats = ps.to_list()
    table = [p.min_score for p in pats]
    bins = steps = step_bins = 0  # final bins, columns, bins written over all gather steps
    for p in pats:
        span = 1
        for w in p.weights:
            span += max(w.acgtn[:4]) - min(w.acgtn[:4])
            step_bins += span
        bins += span
        steps += len(p)
    dev, dev_ms = timed(lambda: ps.pvalue_thresholds(a.pvalue, device=a.device), a.steps, a.warmup)
    res = {"strands": len(pats), "pvalue": a.pvalue, "final_bins": bins, "columns": steps, "step_bins": step_bins,
           "device_ms": round(statistics.median(dev_ms), 3), "device_ms_all": [round(x, 3) for x in dev_ms],
           "scratch_mb": os.environ.get("TFBS_PVALUE_SCRATCH_MB", "256")}
    if not a.skip_host:
        host, host_ms = timed(lambda: ps.pvalue_thresholds(a.pvalue, device=-1), a.steps, a.warmup)
        if host != dev:
            raise SystemExit("device and host thresholds differ")
        res.update(host_ms=round(statistics.median(host_ms), 3), host_ms_all=[round(x, 3) for x in host_ms],
                   host_threads=a.threads)
    diff = [abs(x - y) for x, y in zip(dev, table) if x != y]
    res.update(differs_from_thr_table=len(diff), max_abs_difference=max(diff) if diff else 0)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
