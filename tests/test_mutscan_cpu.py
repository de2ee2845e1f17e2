"""Host side of the mutation scan, no GPU: tfbs_batch_mutscan_tsv against mutscan_ref.format_tsv on
model-made records, the record's layout, the header constant, tfbs_run_ext's growth, the command
line's flags, the host-side error codes, and the condition that makes the GPU cases bite: the model
finds every kind often in each of them.  Integer work and text: every comparison is exact."""
import collections
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dinuc_cases as K
import effects_ref as E
import mutscan_cases as MC
import mutscan_ref as M
from helpers import T, build_batch

CHROM = "7"
E_ARG, E_STATE = -1, -14


def small_case():
    """One region of 40 columns with an N, a mono strand of 4 columns and a dinucleotide strand of 3
    bases on the negative direction, an OtherPattern between them."""
    s, e = 5000, 5033
    lmax = 4
    es, ee = s + 1 - lmax, e + lmax - 1
    ref = ("ACGTTGCANGTCAAGT" * 4)[:ee - es + 1]
    w = [[(7 * i + 3 * j) % 11 - 4 for j in range(4)] for i in range(lmax)]
    rows = [[(5 * i + 3 * j) % 13 - 6 for j in range(16)] for i in range(2)]
    pats = [T.Pattern.PWM([T.Weight(*x) for x in w], "m4", 3, 6), T.Pattern.OtherPattern("other", 4),
            T.Pattern.DiPWM(rows, "d3", 9, 2, T.DIR_N)]
    reg = {"merged": (s, e), "ref": ref, "es": es, "ee": ee, "records": []}
    return {"pats": pats, "n": 2, "regions": [reg], "beds": [("a.bed", [(s, e)])]}


def test_record_layout_and_constants():
    assert C.sizeof(T._capi.tfbs_mutation) == 80
    dt = np.dtype(T.MUTATION_DTYPE)
    assert dt.itemsize == C.sizeof(T._capi.tfbs_mutation)
    assert [n for n, _ in T._capi.tfbs_mutation._fields_] == list(dt.names)
    assert [n for n in dt.names if not n.startswith("reserved")] == list(M.FIELDS)
    for name, _ in T._capi.tfbs_mutation._fields_:
        assert dt.fields[name][1] == getattr(T._capi.tfbs_mutation, name).offset, name
        assert dt.fields[name][0].itemsize == getattr(T._capi.tfbs_mutation, name).size, name
    assert dt.fields["pos"][1] == 16 and dt.fields["ref_start"][1] == 48 and dt.fields["ref_score"][0] == np.dtype("<i4")
    hdr = open(os.path.join(os.path.dirname(T.__file__), "..", "include", "tfbs_amd.h")).read()
    assert "} tfbs_mutation; /* 80 bytes */" in hdr
    assert '#define TFBS_MUTSCAN_HEADER "%s"' % T.MUTSCAN_HEADER.replace("\t", "\\t").replace("\n", "\\n") in hdr
    assert T.MUTSCAN_HEADER == M.HEADER and T.MUTSCAN_HEADER.count("\t") == 15
    for name, bit in (("GAIN", 1), ("LOSS", 2), ("CHANGE", 4), ("SAME", 8), ("NONE", 16), ("SITES", 7), ("ALL", 31)):
        assert "#define TFBS_MUT_%s %d\n" % (name, bit) in hdr and getattr(T, "MUT_" + name) == bit
    assert (M.GAIN, M.LOSS, M.CHANGE, M.SAME, M.NONE, M.SITES, M.ALL) == (1, 2, 4, 8, 16, 7, 31)
    assert T.MUT_KINDS == M.KINDS and T.mutscan_kinds_mask("gain,none") == 17 and T.mutscan_kinds_mask(["same"]) == 8
    Lr = T.mutscan_ring_max_length()
    assert 33 <= Lr <= 129  # the cases stand on both sides of it: strands of Lr, Lr + 1 and 2 Lr + 3 columns


def test_run_ext_grew_at_its_end():
    old, new = T._capi.tfbs_run_ext_pvalue, T._capi.tfbs_run_ext_mutscan
    names = [n for n, _ in new._fields_]
    assert names[:len(old._fields_)] == [n for n, _ in old._fields_]
    assert names[len(old._fields_):] == ["mutscan_output", "mutscan_kinds"]
    for n, _ in old._fields_:  # the earlier layout is a prefix: a caller built against it goes on working
        assert getattr(old, n).offset == getattr(new, n).offset
    assert new.mutscan_output.offset == C.sizeof(old) and new.mutscan_kinds.size == 4
    hdr = open(os.path.join(os.path.dirname(T.__file__), "..", "include", "tfbs_amd.h")).read()
    ext = hdr[hdr.index("typedef struct tfbs_run_ext {"):hdr.index("} tfbs_run_ext;")]
    assert ext.index("pwm_pvalue;") < ext.index("mutscan_output;") < ext.index("mutscan_kinds;")


def test_command_line_flags():
    exe = os.path.join(os.path.dirname(T.__file__), "bin", "find-tfbs-amd")
    r = subprocess.run([exe, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--mutscan_output FILE" in r.stderr and "--mutscan_kinds gain,loss,change,same,none" in r.stderr
    r = subprocess.run([exe, "--mutscan_kinds", "gain,some"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--mutscan_kinds is a comma list" in r.stderr
    r = subprocess.run([exe, "--mutscan_kinds", ""], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2
    r = subprocess.run([exe, "--mutscan_output"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--mutscan_output needs a value" in r.stderr
    r = subprocess.run([exe, "--mutscan_kinds", "gain,loss,change,same,none"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--mutscan_kinds is" not in r.stderr  # (accepted: only the required flags miss)


def test_tsv_against_the_restatement():
    case = small_case()
    pats = case["pats"]
    rows = M.expected(pats, case["regions"])
    kinds = collections.Counter(x[5] for x in rows)
    assert all(kinds[k] > 0 for k in range(5)), kinds
    assert {x[2] for x in rows} == {0, 2}  # no record of the TFBS_KIND_OTHER strand
    assert not any(x[1] == case["regions"][0]["ref"].index("N") for x in rows)  # nor of the N column
    ps = T.PatternSet.from_patterns(pats)
    b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
    want = M.format_tsv(CHROM, pats, case["regions"], rows)
    got = b.mutscan_tsv(M.as_array(rows), CHROM)
    assert got == want
    assert b.mutscan_tsv(M.as_array(rows), CHROM, header=True) == T.MUTSCAN_HEADER + want
    lines = [l.split("\t") for l in got.splitlines()]
    assert len(lines) == len(rows) and all(len(l) == 16 for l in lines)
    assert all(l[0] == CHROM and l[1] == "5000-5033" for l in lines)
    assert {l[5] for l in lines} == set(M.KINDS) and {l[8] for l in lines} == {"+", "-"}
    assert all(int(l[15]) == int(l[14]) - int(l[11]) for l in lines)
    # any subset, in any order: the records are self-contained; and a batch that keeps no variants
    sub = rows[::-3]
    assert b.mutscan_tsv(M.as_array(sub), CHROM) == M.format_tsv(CHROM, pats, case["regions"], sub)
    assert b.mutscan_tsv(M.as_array([]), CHROM) == ""
    plain = build_batch(ps, case["n"], case["beds"], case["regions"])
    assert plain.mutscan_tsv(M.as_array(rows), CHROM) == want
    # a delta beyond int32: a signed 64-bit difference
    x = list(rows[0])
    x[8], x[10] = -(1 << 31), (1 << 31) - 1
    assert b.mutscan_tsv(M.as_array([tuple(x)]), CHROM).rstrip("\n").split("\t")[15] == str((1 << 32) - 1)


def test_host_side_error_codes():
    case = small_case()
    ps = T.PatternSet.from_patterns(case["pats"])
    b = E.build_batch(ps, case["n"], case["beds"], case["regions"])
    rows = M.expected(case["pats"], case["regions"])
    for field, bad in (("region", 1), ("pattern", 3), ("ref", 4), ("alt", 4), ("kind", 5)):
        a = M.as_array(rows[:3])
        a[field][1] = bad
        with pytest.raises(T.TfbsError) as ei:
            b.mutscan_tsv(a, CHROM)
        assert ei.value.code == E_ARG, field
    L = T.lib()
    p, n, n64 = C.c_void_p(), C.c_size_t(), C.c_uint64()
    a = M.as_array(rows[:3])
    assert L.tfbs_batch_mutscan_tsv(None, a.ctypes.data_as(C.c_void_p), 3, b"7", C.byref(p), C.byref(n)) == E_ARG
    assert L.tfbs_batch_mutscan_tsv(b.h, None, 3, b"7", C.byref(p), C.byref(n)) == E_ARG
    assert L.tfbs_batch_mutscan_tsv(b.h, a.ctypes.data_as(C.c_void_p), 3, None, C.byref(p), C.byref(n)) == E_ARG
    # (no ctx without a device: the null checks come first)
    assert L.tfbs_batch_mutscan(None, b.h, 0, 1, T.MUT_ALL, C.byref(p), C.byref(n)) == E_ARG
    assert L.tfbs_batch_mutscan_count(None, b.h, 0, 1, T.MUT_ALL, C.byref(n64)) == E_ARG
    assert L.tfbs_ctx_last_mutscan_ms(None, (C.c_double * 4)()) == E_ARG


def gpu_cases():
    """The cases of test_gpu_mutscan.py's reference equality as (name, patterns, regions)."""
    import test_gpu_effects as TE
    parts = MC.case_edges()
    out = [("edges_" + k, c["pats"], c["regions"]) for k, c in parts.items()]
    for name in ("case_all_kernels", "case_n_and_indels"):
        case = getattr(K, name)()
        out.append((name, TE.case_patterns(case), case["regions"]))
    case = MC.case_special_region()
    out.append(("special", case["pats"], case["regions"]))
    return out


def test_the_gpu_cases_hold_every_kind():
    """At least 20 records of each of the five kinds in case_edges, case_all_kernels,
    case_n_and_indels and the special region: a kernel that never emits one kind cannot pass."""
    per = collections.defaultdict(collections.Counter)
    for name, pats, regions in gpu_cases():
        rows = M.expected(pats, regions, key=name)
        per["case_edges" if name.startswith("edges_") else name].update(x[5] for x in rows)
    assert set(per) == {"case_edges", "case_all_kernels", "case_n_and_indels", "special"}
    for name, kinds in per.items():
        for k in range(5):
            assert kinds[k] >= 20, (name, M.KINDS[k], kinds[k])


def test_edge_case_shapes():
    """case_edges holds what it is there for, seen from the model alone."""
    parts = MC.case_edges()
    Lr = MC.ring_max()
    short, long_ = parts["short"], parts["long"]
    assert tuple(len(r["ref"]) for r in short["regions"]) == MC.EDGE_COLUMNS
    assert sorted(len(p) for p in long_["pats"]) == [64, Lr, Lr + 1, 2 * Lr + 3]
    lens = {(p.kind, len(p)) for p in short["pats"]}
    assert {(T.KIND_PWM, L) for L in (1, 2, 8, 32, 33)} <= lens and {(T.KIND_DIPWM, L) for L in (2, 3, 32)} <= lens
    assert any(p.kind == T.KIND_OTHER for p in short["pats"])
    rows = M.expected(short["pats"], short["regions"], key="edges_short")
    idx = {p.name: i for i, p in enumerate(short["pats"])}
    # every window ties under the all-zero strands: both windows are the lowest one, max(0, c - L + 1)
    for name, kind in (("zero_mono", 3), ("zero_di", 4)):
        mine = [x for x in rows if x[2] == idx[name]]
        L = len(short["pats"][idx[name]])
        assert mine and all(x[5] == kind and x[9] == x[11] == max(0, x[1] - L + 1) for x in mine)
    # the strict >: a reference best equal to min_score does not pass
    p = short["pats"][idx["m8_at_best"]]
    assert any(x[8] == p.min_score and x[5] in (0, 4) for x in rows if x[2] == idx["m8_at_best"])
    # N at column 0, at the chunk boundary, at the last column, as a run of 3 and on both sides of a column
    codes = [K.codes_of(r["ref"]) for r in short["regions"]]
    assert any(c[0] == 4 for c in codes) and any(c[-1] == 4 for c in codes)
    assert any(all(c[k] == 4 for k in (62, 63, 64, 65)) for c in codes if len(c) > 65)
    assert any(c[k] == c[k + 1] == c[k + 2] == 4 for c in codes for k in range(len(c) - 2))
    assert any(c[k] == 4 and c[k + 1] != 4 and c[k + 2] == 4 for c in codes for k in range(len(c) - 2))
    # wrapped sums: weights at INT32_MIN; strands longer than some region
    assert any(w == K.INT32_MIN for p in short["pats"] if p.kind == T.KIND_DIPWM for row in p.weights for w in row)
    assert min(MC.EDGE_COLUMNS) < 32 and min(len(r["ref"]) for r in long_["regions"]) < Lr + 1
    # a column scored in every 64-column chunk of the longest region, under the ring and on the slow path
    rows = M.expected(long_["pats"], long_["regions"], key="edges_long")
    for pi, p in enumerate(long_["pats"]):
        cols = {x[1] // 64 for x in rows if x[2] == pi and x[0] == 2}
        assert cols == {0, 1, 2, 3}, (len(p), cols)
