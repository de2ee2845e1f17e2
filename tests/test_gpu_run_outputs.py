"""The run flow with every secondary output in one run: what the outputs share (the batches'
kept variants, the two rows' POS chains beside the main output's, the write order across shards,
the closing) on the reference fixture.  Each output's text in a run of all seven equals its text
in a run of its own; the oldest tfbs_run_ext layout still reaches the run; a side output that
cannot be opened fails the run as the first of them does."""
import ctypes as C
import os

import pytest

import test_gpu_affinity as F
from helpers import GOLD, TD, T

pytestmark = pytest.mark.gpu

# output -> (run()'s keyword for its path, its other keywords, its header line; None: the main output's #CHROM line)
OUTPUTS = {
    "hits": ("hits_output", {"hits_mode": "all"}, T.HITS_HEADER),
    "best": ("best_output", {"best_mode": "all"}, T.BEST_HEADER),
    "effects": ("effects_output", {"effects_mode": "all"}, T.EFFECTS_HEADER),
    "mutscan": ("mutscan_output", {"mutscan_kinds": T.MUT_ALL}, T.MUTSCAN_HEADER),
    "affinity": ("affinity_output", {"affinity_mode": "all"}, T.AFFINITY_HEADER),
    "scores": ("scores_output", {}, None),
    "affinity_rows": ("affinity_rows_output", {}, None),
}
E_IO = -8  # TFBS_E_IO: what a hits_output in a missing directory gives


def test_run_flow_all_outputs_together(tmp_path):
    if T.device_count() == 0:
        pytest.fail("gpu test without a visible HIP device")
    main_text = open(os.path.join(GOLD, "expected_output_2.vcf")).read()
    chrom_line = main_text[:main_text.index("\n") + 1]
    assert chrom_line.startswith("#CHROM")
    alone = {}
    for name, (key, modes, header) in OUTPUTS.items():
        path = tmp_path / ("alone_%s.gz" % name)
        F.run_fixture(tmp_path / ("alone_%s.vcf.gz" % name), regions_per_batch=512, **{key: str(path)}, **modes)
        alone[name] = T.bgzf_read(str(path))
        header = chrom_line if header is None else header
        assert alone[name].startswith(header) and len(alone[name]) > len(header), name
    for k, kw in enumerate(({"regions_per_batch": 1}, {"devices": [0, 0, 0], "regions_per_batch": 1})):
        args, paths = {}, {}
        for name, (key, modes, _) in OUTPUTS.items():
            paths[name] = str(tmp_path / ("all%d_%s.gz" % (k, name)))
            args[key] = paths[name]
            args.update(modes)
        out = tmp_path / ("all%d.vcf.gz" % k)
        F.run_fixture(out, **args, **kw)
        assert T.bgzf_read(str(out)) == main_text, kw
        for name, path in paths.items():
            assert T.bgzf_read(path) == alone[name], (name, kw)
        assert not [f for f in os.listdir(str(tmp_path)) if f.endswith(".part")], kw

    def args_for(out):
        a = T._capi.tfbs_run_args()
        a.chromosome, a.bcf, a.bed_files = b"chr1", os.path.join(TD, "genotypes2.bcf").encode(), ",".join(F.BEDS).encode()
        a.reference, a.samples_file = os.path.join(TD, "reference_genome.fa").encode(), os.path.join(TD, "samples").encode()
        a.pwm_file, a.pwm_threshold_dir, a.pwm_names = os.path.join(TD, "pwm_definitions.txt").encode(), TD.encode(), b"ACGT"
        a.output, a.pwm_threshold, a.threads = str(out).encode(), 0.0001, 1
        return a

    # the oldest struct: `size` covers effects_output and effects_mode alone
    x = T._capi.tfbs_run_ext()
    x.size = C.sizeof(x)
    assert x.size < C.sizeof(T._capi.tfbs_run_ext_scores)
    x.effects_output, x.effects_mode = str(tmp_path / "old_effects.gz").encode(), T.EFFECT_MODES["all"]
    a = args_for(tmp_path / "old.vcf.gz")
    T.check(T.lib().tfbs_run_ex(C.byref(a), C.byref(x)))
    assert T.bgzf_read(str(tmp_path / "old.vcf.gz")) == main_text
    assert T.bgzf_read(str(tmp_path / "old_effects.gz")) == alone["effects"]

    # a side output that cannot be opened: the last of the table fails as the first does
    missing = tmp_path / "no_such_directory"
    for key in ("hits_output", "affinity_rows_output"):
        with pytest.raises(T.TfbsError) as ei:
            F.run_fixture(tmp_path / ("fail_%s.vcf.gz" % key), **{key: str(missing / "x.gz")})
        print(key, "in a missing directory:", ei.value.code)
        assert ei.value.code == E_IO, key
    assert not os.path.exists(str(missing))
