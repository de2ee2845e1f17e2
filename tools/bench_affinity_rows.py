#!/usr/bin/env python3
"""Times the affinity rows (affinity_rows.hip, tfbs_batch_affinity_rows) on one resident batch.

The two synthetic batches of tools/bench_scores.py (tfbs_synth_fill_batch): the small C2 workload
(1 000 samples x 1 000 regions, 10 PWMs of 8..15 columns, seed 2) and 32 regions of C3's generator
at 50 000 samples with 10 pattern ids (PWMs of 8..30 columns, both strands, seed 3).  In one
process, on the same resident batch, as medians of --steps rounds after --warmup:

  * tfbs_batch_affinity_rows over all regions with the text: the four stages of
    tfbs_ctx_last_affinity_rows_ms -- the affinity kernel, the fold + statistics kernels, the text
    kernel (HIP events on the ctx stream, summed over the scratch chunks), the copy-back + host part
    (wall) -- and the call's wall time;
  * the count-only call's wall time (no text kernel, no text copied back);
  * the rows, the text bytes and the shared text kernel's bytes per second (the genotype text it
    writes), beside the score rows' on the same batch (tfbs_batch_score_rows, tfbs_ctx_last_scores_ms);
  * the affinity kernel's time beside tfbs_batch_affinity's over the same regions in calls of
    --group regions (tools/bench_affinity.py's route: the same kernel, its records copied back).

Prints one JSON line per workload.

  python tools/bench_affinity_rows.py [--steps 5] [--warmup 2] [--workloads C2,C3x32] [--min_spread 1]
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
    "C2": dict(samples=1000, regions=1000, pwms=10, length_config=2, seed=2, threshold=1e-4),
    "C3x32": dict(samples=50000, regions=32, pwms=10, length_config=3, seed=3, threshold=1e-4),
}


def geno_bytes_of(text):
    return sum(len(l) - l.index("\tGT:DS") - 6 for l in text.splitlines())


def run(T, name, w, steps, warmup, min_spread, group):
    work = tempfile.mkdtemp(prefix="tfbs_bench_affinity_rows_")
    names = T.synth_write_pwms(work, w["pwms"], w["length_config"], w["seed"])
    ps = T.parse_pwm_files(os.path.join(work, "pwms.txt"), os.path.join(work, "thr"), w["threshold"], names)
    b = T.RegionBatch(ps, w["samples"], build_device=0)
    b.synth_fill(w["seed"], 0, w["regions"], 0)
    sc = T.Scanner(ps)
    try:
        b.upload(sc)
        groups = [(r0, min(b.num_regions, r0 + group)) for r0 in range(0, b.num_regions, group)]
        stages, wall, count_wall, aff_kernel, score_text = [[], [], [], []], [], [], [], []
        rows = text_bytes = geno_bytes = score_rows = score_geno = None
        for i in range(warmup + steps):
            t0 = time.perf_counter()
            text, n, _ = b.affinity_rows(sc, "chr1", 0, min_spread)
            t1 = time.perf_counter()
            ms = sc.last_affinity_rows_ms()
            c = b.affinity_rows(sc, "chr1", 0, min_spread, fake_position=None)[1]
            t2 = time.perf_counter()
            assert c == n and rows in (None, n)
            rows, text_bytes, geno_bytes = n, len(text), geno_bytes_of(text)
            k_ms = 0.0
            for r0, r1 in groups:
                b.affinity(sc, r0, r1)
                k_ms += sc.last_affinity_ms()[0]
            stext, sn, _ = b.score_rows(sc, "chr1", 0, 1)
            score_rows, score_geno = sn, geno_bytes_of(stext)
            if i >= warmup:
                for k in range(4):
                    stages[k].append(ms[k])
                wall.append((t1 - t0) * 1e3)
                count_wall.append((t2 - t1) * 1e3)
                aff_kernel.append(k_ms)
                score_text.append(sc.last_scores_ms()[2])
        med = lambda xs: round(statistics.median(xs), 4)
        spread = lambda xs: [round(min(xs), 4), round(max(xs), 4)]
        rate = lambda nbytes, xs: round(nbytes / (statistics.median(xs) * 1e-3)) if statistics.median(xs) > 0 else None
        return {
            "tool": "bench_affinity_rows", "workload": name, "samples": w["samples"], "regions": b.num_regions,
            "pwms": w["pwms"], "strands": len(ps), "haplotypes": b.num_haplotypes, "min_spread": min_spread,
            "rows": rows, "text_bytes": text_bytes, "genotype_text_bytes": geno_bytes,
            "affinity_kernel_ms": med(stages[0]), "affinity_kernel_ms_range": spread(stages[0]),
            "fold_and_stats_ms": med(stages[1]), "fold_and_stats_ms_range": spread(stages[1]),
            "text_kernel_ms": med(stages[2]), "text_kernel_ms_range": spread(stages[2]),
            "copy_back_and_host_ms": med(stages[3]), "copy_back_and_host_ms_range": spread(stages[3]),
            "call_wall_ms": med(wall), "count_only_wall_ms": med(count_wall),
            "text_kernel_bytes_per_s": rate(geno_bytes, stages[2]),
            "batch_affinity_kernel_ms": med(aff_kernel), "batch_affinity_kernel_ms_range": spread(aff_kernel),
            "batch_affinity_group": group,
            "score_rows": score_rows, "score_rows_genotype_text_bytes": score_geno,
            "score_rows_text_kernel_ms": med(score_text), "score_rows_text_kernel_bytes_per_s": rate(score_geno, score_text),
            "steps": steps, "warmup": warmup}
    finally:
        sc.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", default="C2,C3x32")
    ap.add_argument("--min_spread", type=int, default=1)
    ap.add_argument("--group", type=int, default=32)
    a = ap.parse_args()
    import tfbs_pkg

    T = tfbs_pkg.load()
    if T.device_count() == 0:
        raise SystemExit("bench_affinity_rows: no HIP device visible")
    for name in a.workloads.split(","):
        print(json.dumps(run(T, name, WORKLOADS[name], a.steps, a.warmup, a.min_spread, a.group)), flush=True)


if __name__ == "__main__":
    main()
