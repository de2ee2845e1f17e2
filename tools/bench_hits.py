#!/usr/bin/env python3
"""Times the hit list kernel (scan_hits.hip) beside the count path's scan on one synthetic batch.

Builds bench.py's C2 workload (1 000 samples x 1 000 regions, seed 2) with C2's pattern set
(10 synthetic PWMs of 8..15 columns, both strands, threshold 1e-4) and reports, as medians
of --steps calls after --warmup:

  * tfbs_batch_hits over all regions: the count pass, the offset scan, the fill pass (HIP
    events on the ctx stream, tfbs_ctx_last_hits_ms) and the copy-back + host part (wall),
    and the whole call's wall time;
  * tfbs_batch_hits_count over all regions (count pass + scan only), wall;
  * the same batch's tfbs_scan (tfbs_ctx_last_scan_ms), the count path's kernel;
  * the number of hits and of (haplotype, strand) pairs and strand-windows scored.

Prints one JSON line.  The kernel scores every window of every distinct haplotype from the
pattern set alone -- no reference-window reuse, no shared windows -- so it does num_windows
strand-windows where the scan does num_scan_windows.

  python tools/bench_hits.py [--steps 20] [--warmup 3] [--samples 1000] [--regions 1000] [--pwms 10]
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

C2 = dict(samples=1000, regions=1000, pwms=10, length_config=2, seed=2, threshold=1e-4)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=C2["samples"])
    ap.add_argument("--regions", type=int, default=C2["regions"])
    ap.add_argument("--pwms", type=int, default=C2["pwms"])
    a = ap.parse_args()
    import tfbs_pkg

    T = tfbs_pkg.load()
    if T.device_count() == 0:
        raise SystemExit("bench_hits: no HIP device visible")
    work = tempfile.mkdtemp(prefix="tfbs_bench_hits_")
    names = T.synth_write_pwms(work, a.pwms, C2["length_config"], C2["seed"])
    ps = T.parse_pwm_files(os.path.join(work, "pwms.txt"), os.path.join(work, "thr"), C2["threshold"], names)
    b = T.RegionBatch(ps, a.samples)
    b.synth_fill(C2["seed"], 0, a.regions, 0)
    sc = T.Scanner(ps)
    try:
        b.upload(sc)
        scan_ms, parts, wall_hits, wall_count = [], [], [], []
        n_hits = None
        ms4 = (C.c_double * 4)()
        for i in range(a.warmup + a.steps):
            b.scan(sc, upload=False, download=False)
            T.check(T.lib().tfbs_ctx_sync(sc.h))
            t0 = time.perf_counter()
            hits = b.hits(sc)
            t1 = time.perf_counter()
            T.check(T.lib().tfbs_ctx_last_hits_ms(sc.h, ms4))
            got = list(ms4)
            t2 = time.perf_counter()
            counts = b.hits_count(sc)
            t3 = time.perf_counter()
            assert n_hits in (None, len(hits)) and int(counts.sum()) == len(hits)
            n_hits = len(hits)
            if i >= a.warmup:
                scan_ms.append(sc.last_scan_ms())
                parts.append(got)
                wall_hits.append((t1 - t0) * 1e3)
                wall_count.append((t3 - t2) * 1e3)
        med = lambda xs: round(statistics.median(xs), 4)
        spread = lambda xs: [round(min(xs), 4), round(max(xs), 4)]
        col = lambda k: [p[k] for p in parts]
        print(json.dumps({
            "tool": "bench_hits", "samples": a.samples, "regions": a.regions, "pwms": a.pwms, "strands": len(ps),
            "haplotypes": b.num_haplotypes, "pairs": b.num_haplotypes * len(ps), "strand_windows": b.num_windows,
            "scan_strand_windows": b.num_scan_windows, "hits": n_hits, "hit_bytes": n_hits * 40,
            "count_pass_ms": med(col(0)), "count_pass_ms_range": spread(col(0)),
            "offset_scan_ms": med(col(1)), "offset_scan_ms_range": spread(col(1)),
            "fill_pass_ms": med(col(2)), "fill_pass_ms_range": spread(col(2)),
            "copy_back_and_host_ms": med(col(3)), "copy_back_and_host_ms_range": spread(col(3)),
            "hits_call_wall_ms": med(wall_hits), "hits_count_call_wall_ms": med(wall_count),
            "tfbs_scan_ms": med(scan_ms), "tfbs_scan_ms_range": spread(scan_ms),
            "count_pass_windows_per_s": b.num_windows / (statistics.median(col(0)) * 1e-3),
            "steps": a.steps, "warmup": a.warmup}))
    finally:
        sc.close()


if __name__ == "__main__":
    main()
