#!/usr/bin/env python3
"""Times the best-site kernel (scan_best.hip) beside the hit list's count pass on one resident batch.

Two synthetic batches (tfbs_synth_fill_batch): bench.py's C3 pattern set and samples (600 PWMs of
8..30 columns, both strands, 50 000 samples, seed 3) on 512 regions, and the small C2 workload
(1 000 samples x 1 000 regions, 10 PWMs of 8..15 columns, seed 2).  In one process, on the same
resident batch, as medians of --steps rounds after --warmup:

  * tfbs_batch_best over all regions, in calls of --group regions so that the dense records held
    at once stay bounded: the kernel (HIP events on the ctx stream, tfbs_ctx_last_best_ms out[0])
    and the copy-back + host part (out[1]), summed over the calls; the calls' wall time;
  * tfbs_batch_hits_count over all regions: the hit list's count pass (tfbs_ctx_last_hits_ms
    out[0]), the same scoring code doing the same scoring work -- the yardstick.  The ratio says
    what the range test, the per-lane maxima and the wave reduction cost on top of it;
  * the records and the bytes copied back (16 per record), the (haplotype, strand) pairs and the
    strand-windows scored.

Prints one JSON line per workload.

  python tools/bench_best.py [--steps 7] [--warmup 2] [--workloads C3,C2] [--group 32]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {  # samples, regions, pwms, length_config, seed, threshold
    "C3": dict(samples=50000, regions=512, pwms=600, length_config=3, seed=3, threshold=1e-4),
    "C2": dict(samples=1000, regions=1000, pwms=10, length_config=2, seed=2, threshold=1e-4),
}


def run(T, name, w, steps, warmup, group):
    work = tempfile.mkdtemp(prefix="tfbs_bench_best_")
    names = T.synth_write_pwms(work, w["pwms"], w["length_config"], w["seed"])
    ps = T.parse_pwm_files(os.path.join(work, "pwms.txt"), os.path.join(work, "thr"), w["threshold"], names)
    b = T.RegionBatch(ps, w["samples"], keep_membership=False)
    b.synth_fill(w["seed"], 0, w["regions"], 0)
    sc = T.Scanner(ps)
    try:
        b.upload(sc)
        kernel, host, wall, count_pass = [], [], [], []
        n_rec = None
        ms4 = (C.c_double * 4)()
        for i in range(warmup + steps):
            k_ms = h_ms = 0.0
            recs = 0
            t0 = time.perf_counter()
            for r0 in range(0, b.num_regions, group):
                recs += len(b.best(sc, r0, min(b.num_regions, r0 + group)))
                ms = sc.last_best_ms()
                k_ms += ms[0]
                h_ms += ms[1]
            t1 = time.perf_counter()
            b.hits_count(sc)
            T.check(T.lib().tfbs_ctx_last_hits_ms(sc.h, ms4))
            assert n_rec in (None, recs)
            n_rec = recs
            if i >= warmup:
                kernel.append(k_ms)
                host.append(h_ms)
                wall.append((t1 - t0) * 1e3)
                count_pass.append(ms4[0])
        med = lambda xs: round(statistics.median(xs), 4)
        spread = lambda xs: [round(min(xs), 4), round(max(xs), 4)]
        n_ranges = sum(len(b.ranges(r)) for r in range(b.num_regions))
        return {
            "tool": "bench_best", "workload": name, "samples": w["samples"], "regions": b.num_regions,
            "pwms": w["pwms"], "strands": len(ps), "haplotypes": b.num_haplotypes,
            "pairs": b.num_haplotypes * len(ps), "strand_windows": b.num_windows, "ranges": n_ranges,
            "records": n_rec, "bytes_copied_back": n_rec * 16, "group": group,
            "best_kernel_ms": med(kernel), "best_kernel_ms_range": spread(kernel),
            "best_copy_back_and_host_ms": med(host), "best_copy_back_and_host_ms_range": spread(host),
            "best_calls_wall_ms": med(wall),
            "hits_count_pass_ms": med(count_pass), "hits_count_pass_ms_range": spread(count_pass),
            "ratio_best_over_count_pass": round(statistics.median(kernel) / statistics.median(count_pass), 4),
            "steps": steps, "warmup": warmup}
    finally:
        sc.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", default="C3,C2")
    ap.add_argument("--group", type=int, default=32)
    a = ap.parse_args()
    import tfbs_pkg

    T = tfbs_pkg.load()
    if T.device_count() == 0:
        raise SystemExit("bench_best: no HIP device visible")
    for name in a.workloads.split(","):
        print(json.dumps(run(T, name, WORKLOADS[name], a.steps, a.warmup, a.group)), flush=True)


if __name__ == "__main__":
    main()
