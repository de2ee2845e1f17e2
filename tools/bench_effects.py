#!/usr/bin/env python3
"""Times the variant-effect path (scan_effects.hip) on C2's batch, the best-site kernel beside it.

The small C2 workload (1 000 samples x 1 000 regions, 10 PWMs of 8..15 columns, both strands,
seed 2) through tfbs_synth_fill_batch with the variants kept.  In one process, as medians of
--steps rounds after --warmup:

  * tfbs_batch_effects over all regions in one call: the host's patching and packing, the kernel
    (HIP events on the ctx stream) and the copy-back + host expansion (tfbs_ctx_last_effects_ms),
    and the call's wall time;
  * tfbs_batch_best over the same batch, resident, in calls of --group regions: its kernel time
    (tfbs_ctx_last_best_ms out[0]) for scale -- the same scoring code on every window of every
    distinct haplotype;
  * the records, the scored records, the (scored record, strand) pairs, the strand-windows the
    kernel scores (n_ref + n_alt summed over the records) and strand-windows per second of kernel
    time.

Prints one JSON line.

  python tools/bench_effects.py [--steps 20] [--warmup 3] [--group 32]
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

C2 = dict(samples=1000, regions=1000, pwms=10, length_config=2, seed=2, threshold=1e-4)


def run(T, w, steps, warmup, group):
    work = tempfile.mkdtemp(prefix="tfbs_bench_effects_")
    names = T.synth_write_pwms(work, w["pwms"], w["length_config"], w["seed"])
    ps = T.parse_pwm_files(os.path.join(work, "pwms.txt"), os.path.join(work, "thr"), w["threshold"], names)
    b = T.RegionBatch(ps, w["samples"], keep_membership=False, keep_variants=True)
    b.synth_fill(w["seed"], 0, w["regions"], 0)
    sc = T.Scanner(ps)
    try:
        b.upload(sc)  # (the best-site kernel's; the effects need none)
        prep, kernel, host, wall, best_kernel = [], [], [], [], []
        eff = None
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            eff = b.effects(sc)
            t1 = time.perf_counter()
            ms = sc.last_effects_ms()
            k_ms = 0.0
            for r0 in range(0, b.num_regions, group):
                b.best(sc, r0, min(b.num_regions, r0 + group))
                k_ms += sc.last_best_ms()[0]
            if i >= warmup:
                prep.append(ms[0])
                kernel.append(ms[1])
                host.append(ms[2])
                wall.append((t1 - t0) * 1e3)
                best_kernel.append(k_ms)
        med = lambda xs: round(statistics.median(xs), 4)
        spread = lambda xs: [round(min(xs), 4), round(max(xs), 4)]
        scored = eff[eff["status"] == T.VAR_SCORED]
        windows = int(scored["n_ref"].astype("u8").sum() + scored["n_alt"].astype("u8").sum())
        return {
            "tool": "bench_effects", "workload": "C2", "samples": w["samples"], "regions": b.num_regions,
            "pwms": w["pwms"], "strands": len(ps), "records": len(eff) // len(ps),
            "scored_records": len(scored) // len(ps), "pairs": len(scored), "effect_records": len(eff),
            "strand_windows": windows, "bytes_copied_back": len(scored) * 32,
            "host_prep_ms": med(prep), "host_prep_ms_range": spread(prep),
            "kernel_ms": med(kernel), "kernel_ms_range": spread(kernel),
            "copy_back_and_host_ms": med(host), "copy_back_and_host_ms_range": spread(host),
            "call_wall_ms": med(wall),
            "strand_windows_per_s": round(windows / (statistics.median(kernel) * 1e-3)),
            "best_kernel_ms": med(best_kernel), "best_kernel_ms_range": spread(best_kernel),
            "best_strand_windows": b.num_windows, "group": group, "steps": steps, "warmup": warmup}
    finally:
        sc.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--group", type=int, default=32)
    a = ap.parse_args()
    import tfbs_pkg

    T = tfbs_pkg.load()
    if T.device_count() == 0:
        raise SystemExit("bench_effects: no HIP device visible")
    print(json.dumps(run(T, C2, a.steps, a.warmup, a.group)), flush=True)


if __name__ == "__main__":
    main()
