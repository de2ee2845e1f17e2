#!/usr/bin/env python3
"""Times the mutation scan (scan_mutscan.hip) on C2's batch, the variant-effect path beside it.

The small C2 workload (1 000 samples x 1 000 regions, 10 PWMs of 8..15 columns, both strands,
seed 2) through tfbs_synth_fill_batch with the variants kept.  In one process, as medians of
--steps rounds after --warmup:

  * tfbs_batch_mutscan with kinds gain | loss over all regions in one call: the host's packing,
    the count pass + offset scan, the fill pass (HIP events on the ctx stream) and the copy-back +
    host expansion (tfbs_ctx_last_mutscan_ms), and the call's wall time;
  * the same with all five kinds over the first --all_regions regions (every (substitution,
    strand) pair becomes an 80-byte record: the whole batch's would be more than a gigabyte);
  * the (substitution, strand) pairs scored and pairs per second of device time and of wall time;
  * the baseline, the only way to these numbers without the kernel: tfbs_batch_effects on a batch
    whose records are every substitution of the first --baseline_regions regions, one SNV record
    each; its three stages (tfbs_ctx_last_effects_ms) and its pairs per second.

Prints one JSON line.

  python tools/bench_mutscan.py [--steps 20] [--warmup 3] [--all_regions 100] [--baseline_regions 20]
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
NUC = "ACGT"


def med(xs):
    return round(statistics.median(xs), 4)


def spread(xs):
    return [round(min(xs), 4), round(max(xs), 4)]


def time_mutscan(T, sc, b, r1, kinds, steps, warmup):
    stages, wall = [[], [], [], []], []
    n = 0
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        n = len(b.mutscan(sc, 0, r1, kinds=kinds))
        t1 = time.perf_counter()
        ms = sc.last_mutscan_ms()
        if i >= warmup:
            for k in range(4):
                stages[k].append(ms[k])
            wall.append((t1 - t0) * 1e3)
    pairs = b.mutscan_count(sc, 0, r1, kinds=T.MUT_ALL)  # every (substitution, strand) that has a window
    device = statistics.median(stages[1]) + statistics.median(stages[2])
    out = {"regions": r1, "records": n, "pairs": pairs, "call_wall_ms": med(wall),
           "pairs_per_s_device": round(pairs / (device * 1e-3)),
           "pairs_per_s_wall": round(pairs / (statistics.median(wall) * 1e-3))}
    for k, name in enumerate(("host_pack_ms", "count_and_scan_ms", "fill_ms", "copy_back_and_host_ms")):
        out[name] = med(stages[k])
        out[name + "_range"] = spread(stages[k])
    return out


def baseline(T, sc, ps, w, regions, steps, warmup):
    """tfbs_batch_effects on every substitution of the first `regions` regions as SNV records."""
    b = T.RegionBatch(ps, 2, keep_membership=False, keep_variants=True)
    b.add_bed("synthetic.bed")
    subs = 0
    for j in range(regions):
        r = T.SynthRegion(w["seed"], j, w["samples"], ps.max_length, 0)
        b.begin(r.merged[0], r.merged[1], r.ref)
        b.add_inner(0, *r.merged)
        for c, ch in enumerate(r.ref):
            if ch not in NUC:
                continue
            for k in range(1, 4):  # the three other bases, each on a haplotype id of its own
                b.add_record_carriers(r.ext_start + c, ch, NUC[(NUC.index(ch) + k) % 4], [k - 1])
                subs += 1
        b.end()
    stages, wall = [[], [], []], []
    pairs = 0
    for i in range(warmup + steps):
        t0 = time.perf_counter()
        eff = b.effects(sc)
        t1 = time.perf_counter()
        ms = sc.last_effects_ms()
        pairs = int(((eff["status"] == T.VAR_SCORED) & (eff["n_ref"] > 0)).sum())
        if i >= warmup:
            for k in range(3):
                stages[k].append(ms[k])
            wall.append((t1 - t0) * 1e3)
    out = {"regions": regions, "substitutions": subs, "pairs": pairs, "call_wall_ms": med(wall),
           "pairs_per_s_device": round(pairs / (statistics.median(stages[1]) * 1e-3)),
           "pairs_per_s_wall": round(pairs / (statistics.median(wall) * 1e-3))}
    for k, name in enumerate(("host_prep_ms", "kernel_ms", "copy_back_and_host_ms")):
        out[name] = med(stages[k])
        out[name + "_range"] = spread(stages[k])
    return out


def run(T, w, steps, warmup, all_regions, baseline_regions):
    work = tempfile.mkdtemp(prefix="tfbs_bench_mutscan_")
    names = T.synth_write_pwms(work, w["pwms"], w["length_config"], w["seed"])
    ps = T.parse_pwm_files(os.path.join(work, "pwms.txt"), os.path.join(work, "thr"), w["threshold"], names)
    b = T.RegionBatch(ps, w["samples"], keep_membership=False, keep_variants=True)
    b.synth_fill(w["seed"], 0, w["regions"], 0)
    sc = T.Scanner(ps)
    try:
        sites = time_mutscan(T, sc, b, b.num_regions, T.MUT_GAIN | T.MUT_LOSS, steps, warmup)
        every = time_mutscan(T, sc, b, min(all_regions, b.num_regions), T.MUT_ALL, steps, warmup)
        base = baseline(T, sc, ps, w, min(baseline_regions, b.num_regions), steps, warmup)
        return {"tool": "bench_mutscan", "workload": "C2", "samples": w["samples"], "regions": b.num_regions,
                "pwms": w["pwms"], "strands": len(ps), "ring_max_length": T.mutscan_ring_max_length(),
                "gain_loss": sites, "all_kinds": every, "effects_baseline": base,
                "device_speedup_per_pair": round(sites["pairs_per_s_device"] / base["pairs_per_s_device"], 2),
                "wall_speedup_per_pair": round(sites["pairs_per_s_wall"] / base["pairs_per_s_wall"], 2),
                "steps": steps, "warmup": warmup}
    finally:
        sc.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--all_regions", type=int, default=100)
    ap.add_argument("--baseline_regions", type=int, default=20)
    a = ap.parse_args()
    import tfbs_pkg

    T = tfbs_pkg.load()
    if T.device_count() == 0:
        raise SystemExit("bench_mutscan: no HIP device visible")
    print(json.dumps(run(T, C2, a.steps, a.warmup, a.all_regions, a.baseline_regions)), flush=True)


if __name__ == "__main__":
    main()
