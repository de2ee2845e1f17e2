#!/usr/bin/env python3
"""Times the binding-affinity kernel (scan_affinity.hip) beside the best-site kernel on one resident batch.

The synthetic C2 workload of bench.py (tfbs_synth_fill_batch: 1 000 samples x 1 000 regions, 10
PWMs of 8..15 columns, both strands, seed 2); C3's pattern set and samples on 512 regions on
request.  In one process, on the same resident batch, as medians of --steps rounds after --warmup:

  * tfbs_batch_affinity over all regions, in calls of --group regions so that the dense records
    held at once stay bounded: the kernel (HIP events on the ctx stream, tfbs_ctx_last_affinity_ms
    out[0]) and the copy-back + host part (out[1]), summed over the calls; the calls' wall time;
  * tfbs_batch_best over the same groups (tfbs_ctx_last_best_ms): the same walk and the same
    scoring without the weight -- the yardstick.  The ratio says what d, the LDS lookup and the
    64-bit multiply of the windows within the cutoff, and the wider per-lane state cost on top;
  * the records and the bytes copied back (16 per record), the (haplotype, strand) pairs, the
    strand-windows scored, and of the windows counted in a range the share with a weight above 0
    (the lanes that take the lookup).

Prints one JSON line per workload.

  python tools/bench_affinity.py [--steps 20] [--warmup 2] [--workloads C2] [--group 32]
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

WORKLOADS = {  # samples, regions, pwms, length_config, seed, threshold
    "C3": dict(samples=50000, regions=512, pwms=600, length_config=3, seed=3, threshold=1e-4),
    "C2": dict(samples=1000, regions=1000, pwms=10, length_config=2, seed=2, threshold=1e-4),
}


def run(T, name, w, steps, warmup, group):
    work = tempfile.mkdtemp(prefix="tfbs_bench_affinity_")
    names = T.synth_write_pwms(work, w["pwms"], w["length_config"], w["seed"])
    ps = T.parse_pwm_files(os.path.join(work, "pwms.txt"), os.path.join(work, "thr"), w["threshold"], names)
    b = T.RegionBatch(ps, w["samples"], keep_membership=False)
    b.synth_fill(w["seed"], 0, w["regions"], 0)
    sc = T.Scanner(ps)
    try:
        b.upload(sc)
        groups = [(r0, min(b.num_regions, r0 + group)) for r0 in range(0, b.num_regions, group)]
        kernel, host, wall, best_kernel = [], [], [], []
        n_rec = windows = nonzero = None
        for i in range(warmup + steps):
            k_ms = h_ms = bk_ms = 0.0
            recs = nw = nz = 0
            t0 = time.perf_counter()
            for r0, r1 in groups:
                a = b.affinity(sc, r0, r1)
                ms = sc.last_affinity_ms()
                k_ms += ms[0]
                h_ms += ms[1]
                recs += len(a)
                nw += int(a["n_windows"].sum())
                nz += int(a["n_nonzero"].sum())
            t1 = time.perf_counter()
            for r0, r1 in groups:
                b.best(sc, r0, r1)
                bk_ms += sc.last_best_ms()[0]
            assert n_rec in (None, recs) and windows in (None, nw) and nonzero in (None, nz)
            n_rec, windows, nonzero = recs, nw, nz
            if i >= warmup:
                kernel.append(k_ms)
                host.append(h_ms)
                wall.append((t1 - t0) * 1e3)
                best_kernel.append(bk_ms)
        med = lambda xs: round(statistics.median(xs), 4)
        spread = lambda xs: [round(min(xs), 4), round(max(xs), 4)]
        n_ranges = sum(len(b.ranges(r)) for r in range(b.num_regions))
        return {
            "tool": "bench_affinity", "workload": name, "samples": w["samples"], "regions": b.num_regions,
            "pwms": w["pwms"], "strands": len(ps), "haplotypes": b.num_haplotypes,
            "pairs": b.num_haplotypes * len(ps), "strand_windows": b.num_windows, "ranges": n_ranges,
            "records": n_rec, "bytes_copied_back": n_rec * 16, "group": group,
            "windows_in_ranges": windows, "windows_nonzero": nonzero,
            "nonzero_share": round(nonzero / windows, 6) if windows else None,
            "affinity_kernel_ms": med(kernel), "affinity_kernel_ms_range": spread(kernel),
            "affinity_copy_back_and_host_ms": med(host), "affinity_copy_back_and_host_ms_range": spread(host),
            "affinity_calls_wall_ms": med(wall),
            "best_kernel_ms": med(best_kernel), "best_kernel_ms_range": spread(best_kernel),
            "ratio_affinity_over_best": round(statistics.median(kernel) / statistics.median(best_kernel), 4),
            "steps": steps, "warmup": warmup}
    finally:
        sc.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", default="C2")
    ap.add_argument("--group", type=int, default=32)
    a = ap.parse_args()
    import tfbs_pkg

    T = tfbs_pkg.load()
    if T.device_count() == 0:
        raise SystemExit("bench_affinity: no HIP device visible")
    for name in a.workloads.split(","):
        print(json.dumps(run(T, name, WORKLOADS[name], a.steps, a.warmup, a.group)), flush=True)


if __name__ == "__main__":
    main()
