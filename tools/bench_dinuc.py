#!/usr/bin/env python3
"""Times scan_dinuc_kernel against scan_fast_kernel on one synthetic batch.

Builds the regions of bench.py's C2 workload (1 000 samples x 1 000 regions, seed 2) and
times, with the HIP events around tfbs_scan (tfbs_ctx_last_scan_ms), over those regions:

  (a) N synthetic dinucleotide PWMs of base lengths 8..15, both strands
      (scan_dinuc_kernel: ceil((L - 1) / (k - 1)) lookups per four strand-windows);
  (b) N mono PWMs of the same lengths with TFBS_MFMA=0 (scan_fast_kernel, the LUT kernel:
      ceil(L / 4) lookups per eight or four strand-windows) -- the yardstick.

Both sets have the same strand lengths, so both scans score the same strand-windows.
Prints one JSON line: windows/s of each and their ratio.  The dinucleotide kernel's lookup
width k is a build-time constant of the library (TFBS_DINUC_K, Makefile DINUC_K); run the
tool once per build (TFBS_LIB=<path to the other build's libtfbs_amd.so> for the second).

  python tools/bench_dinuc.py [--pwms 10] [--steps 20] [--warmup 3]
"""
import argparse
import json
import math
import os
import random
import statistics
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C2 = dict(samples=1000, regions=1000, length_config=2, seed=2)


def synth_dipwm(rnd, L, name, pid, T, p_hit=1e-4):
    """Random weights in +-2000, both strands; min_score at the p_hit normal quantile of the
    score of a random window (the terms taken as independent): hits as rare as the mono set's."""
    rows = [[rnd.randint(-2000, 2000) for _ in range(16)] for _ in range(L - 1)]
    mean = sum(sum(r) / 16.0 for r in rows)
    var = sum(sum(x * x for x in r) / 16.0 - (sum(r) / 16.0) ** 2 for r in rows)
    z = statistics.NormalDist().inv_cdf(1.0 - p_hit)
    thr = int(mean + z * math.sqrt(var))
    rev = [[rows[L - 2 - i][4 * (3 - b) + (3 - a)] for a in range(4) for b in range(4)] for i in range(L - 1)]
    return [T.Pattern.DiPWM(rows, name, pid, thr, T.DIR_P), T.Pattern.DiPWM(rev, name, pid, thr, T.DIR_N)]


def time_scan(T, ps, n_samples, n_regions, seed, steps, warmup, lmax):
    b = T.RegionBatch(ps, n_samples, keep_membership=False, window_lmax=lmax)
    b.synth_fill(seed, 0, n_regions, 0)
    sc = T.Scanner(ps)
    try:
        ms = []
        for i in range(warmup + steps):
            b.scan(sc, upload=(i == 0), download=False)
            T.check(T.lib().tfbs_ctx_sync(sc.h))
            if i >= warmup:
                ms.append(sc.last_scan_ms())
        launches = T.lib().tfbs_ctx_last_scan_launches(sc.h)
    finally:
        sc.close()
    return b, ms, launches


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pwms", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=C2["samples"])
    ap.add_argument("--regions", type=int, default=C2["regions"])
    a = ap.parse_args()
    os.environ["TFBS_MFMA"] = "0"  # (b) on the LUT kernel; (a) never uses the matrix cores
    import tfbs_pkg

    T = tfbs_pkg.load()
    if T.device_count() == 0:
        raise SystemExit("bench_dinuc: no HIP device visible")
    probe = T.PatternSet.from_patterns([T.Pattern.DiPWM([[0] * 16] * 2, "probe", 0, 0)])
    k = {1024: 3, 16384: 5}[probe.dinuc_stats()["lut_bytes"]]  # one block of 4^k codes x 16 bytes
    work = tempfile.mkdtemp(prefix="tfbs_bench_dinuc_")
    names = T.synth_write_pwms(work, a.pwms, C2["length_config"], C2["seed"])
    mono = T.parse_pwm_files(os.path.join(work, "pwms.txt"), os.path.join(work, "thr"), 1e-4, names)
    rnd = random.Random(C2["seed"])
    dl = []
    for p in mono.to_list():
        if p.direction == T.DIR_P:
            dl += synth_dipwm(rnd, len(p), "DI_" + p.name, p.pattern_id, T)
    di = T.PatternSet.from_patterns(dl)
    assert sorted(len(p) for p in dl) == sorted(len(p) for p in mono.to_list())
    lmax = max(mono.max_length, di.max_length)
    bm, ms_mono, l_mono = time_scan(T, mono, a.samples, a.regions, C2["seed"], a.steps, a.warmup, lmax)
    windows = bm.num_windows  # strand-windows of the carried haplotypes: the same for both sets
    haps = bm.num_haplotypes
    del bm
    bd, ms_di, l_di = time_scan(T, di, a.samples, a.regions, C2["seed"], a.steps, a.warmup, lmax)
    assert bd.num_haplotypes == haps
    md, mm = statistics.median(ms_di), statistics.median(ms_mono)
    st = di.dinuc_stats()
    print(json.dumps({
        "tool": "bench_dinuc", "dinuc_k": k, "pwms": a.pwms, "strands": len(dl), "lengths": sorted(len(p) for p in dl),
        "samples": a.samples, "regions": a.regions, "haplotypes": haps, "strand_windows": windows,
        "dinuc_tiles": st["n_tiles"], "dinuc_lut_bytes": st["lut_bytes"],
        "mono_plan": {k_: v for k_, v in mono.plan_stats(mfma=False).items() if "mfma" not in k_},
        "dinuc_ms": round(md, 4), "dinuc_ms_min": round(min(ms_di), 4), "dinuc_ms_max": round(max(ms_di), 4),
        "fast_ms": round(mm, 4), "fast_ms_min": round(min(ms_mono), 4), "fast_ms_max": round(max(ms_mono), 4),
        "dinuc_windows_per_s": windows / (md * 1e-3), "fast_windows_per_s": windows / (mm * 1e-3),
        "dinuc_over_fast_time": round(md / mm, 3), "launches": {"dinuc": l_di, "fast": l_mono},
        "steps": a.steps, "warmup": a.warmup}))


if __name__ == "__main__":
    main()
