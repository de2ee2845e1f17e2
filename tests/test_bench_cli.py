"""bench.py's command line: a plain run prints the headline line and nothing that
needs runs of its own, --full adds the other legs, --steps sets the timed steps,
and --dump-outputs writes the last step's result -- the same arrays from run to
run, and the counts the library gives for the same batch built here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--workload", "C2", "--regions", "200"]  # 1 000 samples x 200 regions x 10 PWMs
PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "value_note", "step", "ranks", "scanned_windows_per_s",
              "scan_regions_per_s", "effective_windows_per_s"}
FULL_KEYS = {"step_device_ms", "end_to_end", "kernel_ms_avg", "dense_download_s", "roofline", "hbm_roofline",
             "vs_valu_peak", "cpu_baseline"}
DUMP_NAMES = {"region_num_keys", "region_key_digests", "sample_key_ids", "sample_key_counts"}


def _args(monkeypatch, argv):
    import bench

    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "3"]
    r = subprocess.run(cmd + SMALL + list(extra), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(str(d), f)) for f in sorted(os.listdir(str(d)))}


def test_full_and_dump_are_off_by_default(monkeypatch):
    a = _args(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    a = _args(monkeypatch, ["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path, monkeypatch):
    import bench

    line = _bench("--dump-outputs", str(tmp_path / "a"))
    again = _bench("--dump-outputs", str(tmp_path / "b"))
    assert set(line) == PLAIN_KEYS
    assert line["steps"] == 4 and line["warmup"] == 3 and line["n_gpus"] == 1
    assert line["metric"] == "haplotype-windows scored/sec" and line["unit"] == "windows/s"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    assert line["dtype"] == ("fp4xfp6->f32 bound + int32 exact" if line["config"]["scan_path"] == "mfma" else "int32")
    assert line["value"] == pytest.approx(line["config"]["windows_per_step"] * 1e3 / line["ms_per_step"], rel=1e-9)
    got, rep = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(got) == set(rep) == DUMP_NAMES
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    for name in DUMP_NAMES:
        assert got[name].dtype in (np.float32, np.float64), name
        assert got[name].shape == rep[name].shape and np.array_equal(got[name], rep[name]), name
    # the same batch built, scanned and reduced here
    a = _args(monkeypatch, SMALL)
    names = T.synth_write_pwms(str(tmp_path), a.pwms, a.length_config, a.seed)
    ps = T.parse_pwm_files(str(tmp_path / "pwms.txt"), str(tmp_path / "thr"), a.threshold, names)
    b = bench.shard_batch(T, ps, a, 0)
    sc = T.Scanner(ps)
    try:
        b.scan(sc, reduce=True)
        assert line["config"]["windows_per_step"] == b.num_windows
        assert got["region_num_keys"].shape == (a.regions,)
        assert got["region_key_digests"].shape == (a.regions, 2)
        dk, _, _ = b.region_digests(rows=False)
        hi, lo = (got["region_key_digests"][:, i].astype(np.uint64) for i in (0, 1))
        assert np.array_equal((hi << np.uint64(32)) | lo, dk)
        ids, counts = got["sample_key_ids"], got["sample_key_counts"]
        assert ids.shape == (len(counts), 5) and counts.shape[1:] == (2, a.samples)
        sampled = sorted({int(r) for r in ids[:, 0]})
        assert 1 <= len(sampled) <= bench.DUMP_REGIONS_MAX and counts.sum() > 0
        want_n = []
        for r in range(a.regions):
            keys = b.keys_np(r)
            want_n.append(len(keys))
            if r not in sampled:
                continue
            rows = [i for i in range(len(ids)) if int(ids[i, 0]) == r]
            assert len(rows) == len(keys)
            for i, ((bed, (s, e), pid), (left, right)) in zip(rows, keys.items()):
                assert tuple(int(x) for x in ids[i]) == (r, b.beds.index(bed), s, e, pid)
                assert np.array_equal(counts[i, 0], left) and np.array_equal(counts[i, 1], right)
        assert [int(x) for x in got["region_num_keys"]] == want_n
    finally:
        sc.close()


@pytest.mark.gpu
def test_full_run_keeps_every_leg(tmp_path):
    line = _bench("--full", "--cpu-seconds", "0.2", "--dump-outputs", str(tmp_path / "d"))
    assert set(line) == PLAIN_KEYS | FULL_KEYS
    assert set(_load(tmp_path / "d")) == DUMP_NAMES
    assert line["steps"] == 4 and line["ms_per_step"] > 0
    assert line["end_to_end"]["rows"] > 0 and line["end_to_end"]["regions_per_s"] > 0
    assert line["cpu_baseline"]["value"] > 0 and line["step_device_ms"]["scan"] > 0
    assert line["roofline"]["frac"] > 0 and line["hbm_roofline"]["frac"] > 0
