// find-tfbs-amd: the find-tfbs command line (main.rs:163-232) over tfbs_run_ex.
// Long flags are the reference's; the short ones it binds twice (-n, -t,
// main.rs:174/179, 177/181) are accepted in their first meaning only.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/tfbs_amd.h"

static void usage() {
    fprintf(stderr,
            "find-tfbs-amd 1.0.1 (MI355X)\nFind patterns in a VCF file\n\n"
            "USAGE: find-tfbs-amd --chromosome CHROM --input IN --output OUT --reference REF --bed BED[,BED..]\n"
            "       --pwm_names N1[,N2..] --pwm_file PWM (--pwm_threshold_directory DIR --pwm_threshold T | --pwm_pvalue P)\n"
            "       [--dipwm_file DIPWM] [--hits_output FILE [--hits_mode all|diff]]\n"
            "       [--best_output FILE [--best_mode all|diff]]\n"
            "       [--effects_output FILE [--effects_mode sites|all]]\n"
            "       [--scores_output FILE [--scores_min_spread N]]\n"
            "       [--mutscan_output FILE [--mutscan_kinds gain,loss,change,same,none]]\n"
            "       [--affinity_output FILE [--affinity_mode all|diff]]\n"
            "       [--affinity_rows_output FILE [--affinity_rows_min_spread N]]\n"
            "       [--forward_only] [--threads N] [--min_maf N] [--after_position P] [--samples FILE]\n"
            "       [--tabix] [--verbose] [--device D | --devices D1,D2,.. | --gpus N] [--regions_per_batch N]\n"
            "  --devices: one contiguous block of merged regions per listed HIP device (a device may repeat);\n"
            "  --gpus N: devices 0..N-1.  The output is the same for any device list.\n"
            "  --pwm_pvalue P (0 < P < 1): every named definition loads and each strand's threshold is the exact one\n"
            "  of p-value P under a uniform background (the largest top set of scores with probability <= P),\n"
            "  computed on the run's first device; --pwm_threshold_directory and --pwm_threshold are then not\n"
            "  required, and ignored when given.\n"
            "  --dipwm_file: dinucleotide PWMs (rows of 16 weights, AA AC .. TT); --pwm_file is then optional\n"
            "  and --pwm_names selects from both files.\n"
            "  --hits_output FILE: also write where the sites are, as BGZF TSV: per merged region and distinct\n"
            "  haplotype its matches (pattern, strand, range, score).  --hits_mode all: one `hit` line per match;\n"
            "  diff (default): per haplotype a `hap` line with its carrier ids, the most carried haplotype's\n"
            "  matches as `base` lines, the others' `gain` and `loss` lines against it.  --output is unchanged.\n"
            "  --best_output FILE: also write how strongly each haplotype binds, as BGZF TSV: per (bed, inner range),\n"
            "  pattern_id and distinct haplotype the best-scoring site whatever the threshold (strand, range, score).\n"
            "  --best_mode all: one `best` line each; diff (default): `hap` lines, then where a haplotype's best\n"
            "  score differs from the most carried haplotype's a `base` line and `alt` lines with the score's delta.\n"
            "  --effects_output FILE: also write which variant does it, as BGZF TSV: per merged region and record a\n"
            "  `var` line, then per pattern strand the best site touching the record on the REF and on the ALT allele\n"
            "  (range, score) and the score's delta.  --effects_mode sites (default): the `gain`, `loss` and `change`\n"
            "  lines (a side passes above the strand's threshold); all: `same` and `none` lines too.\n"
            "  --scores_output FILE: also write how strongly each sample binds, as a second BGZF VCF: per (bed, inner\n"
            "  range) and pattern_id one row whose per-sample GT:DS comes from the sum of the sample's two haplotypes'\n"
            "  best scores (INFO SCORES=<lowest>,<highest>), whatever the threshold; rows whose sums span less than\n"
            "  --scores_min_spread N (milli-log-odds, default 1) are left out.  --min_maf applies to both files.\n"
            "  --mutscan_output FILE: also write which substitutions would create or destroy a site, as BGZF TSV: per\n"
            "  merged region, pattern strand, reference base and other base the best site covering the base before and\n"
            "  after the substitution (range, score) and the score's delta, whatever the BCF holds.\n"
            "  --mutscan_kinds: the kinds of lines written, a comma list (default gain,loss).\n"
            "  --affinity_output FILE: also write each haplotype's total binding affinity, as BGZF TSV: per (bed, inner\n"
            "  range), pattern_id and distinct haplotype the sum over every window of floor(2^40 exp((score - top) / 1000)),\n"
            "  top the pattern_id's highest possible score: exact integers, ln(affinity) = top / 1000 + ln(sum) - 40 ln 2.\n"
            "  --affinity_mode all: one `aff` line each; diff (default): `hap` lines, then where a haplotype's sum\n"
            "  differs from the most carried haplotype's a `base` line and `alt` lines with the sum's delta.\n"
            "  --affinity_rows_output FILE: also write each sample's total binding affinity, as a further BGZF VCF: per\n"
            "  (bed, inner range) and pattern_id one row whose per-sample GT:DS comes from floor(1000 log2) of the sum of\n"
            "  the sample's two haplotypes' affinities (INFO LOG2AFF=<lowest>,<highest>;AFF=<their sums>;TOP=<top>); rows\n"
            "  whose logarithms span less than --affinity_rows_min_spread N (milli-bits, default 1) are left out.\n"
            "  --min_maf applies.\n");
}

// A flag that takes one of two words: the word's code, or the error and exit status 2.
static int mode_flag(const char *name, const std::string &value, const char *word0, int code0, const char *word1, int code1) {
    if (value == word0) return code0;
    if (value == word1) return code1;
    fprintf(stderr, "error: %s is %s or %s\n", name, word0, word1);
    exit(2);
}

int main(int argc, char **argv) {
    tfbs_run_args a;
    memset(&a, 0, sizeof a);
    a.threads = 1;
    a.hits_mode = TFBS_HITS_DIFF;
    a.best_mode = TFBS_BEST_DIFF;
    tfbs_run_ext x;
    memset(&x, 0, sizeof x);
    x.size = (uint32_t)sizeof x;
    x.effects_mode = TFBS_EFFECTS_SITES;
    x.affinity_mode = TFBS_AFFINITY_DIFF;
    bool have_thr = false;
    std::string gpus;
    for (int i = 1; i < argc; i++) {
        std::string k = argv[i];
        auto val = [&](const char *name) -> const char * {
            if (i + 1 >= argc) {
                fprintf(stderr, "error: %s needs a value\n", name);
                exit(2);
            }
            return argv[++i];
        };
        if (k == "--chromosome" || k == "-c") a.chromosome = val("--chromosome");
        else if (k == "--input" || k == "-i") a.bcf = val("--input");
        else if (k == "--output" || k == "-o") a.output = val("--output");
        else if (k == "--reference" || k == "-r") a.reference = val("--reference");
        else if (k == "--bed" || k == "-b") a.bed_files = val("--bed");
        else if (k == "--pwm_names" || k == "-n") a.pwm_names = val("--pwm_names");
        else if (k == "--pwm_file" || k == "-p") a.pwm_file = val("--pwm_file");
        else if (k == "--dipwm_file") a.dipwm_file = val("--dipwm_file");
        else if (k == "--hits_output") a.hits_output = val("--hits_output");
        else if (k == "--hits_mode") a.hits_mode = mode_flag("--hits_mode", val("--hits_mode"), "all", TFBS_HITS_ALL, "diff", TFBS_HITS_DIFF);
        else if (k == "--best_output") a.best_output = val("--best_output");
        else if (k == "--best_mode") a.best_mode = mode_flag("--best_mode", val("--best_mode"), "all", TFBS_BEST_ALL, "diff", TFBS_BEST_DIFF);
        else if (k == "--effects_output") x.effects_output = val("--effects_output");
        else if (k == "--effects_mode") x.effects_mode = mode_flag("--effects_mode", val("--effects_mode"), "sites", TFBS_EFFECTS_SITES, "all", TFBS_EFFECTS_ALL);
        else if (k == "--mutscan_output") x.mutscan_output = val("--mutscan_output");
        else if (k == "--mutscan_kinds") {
            const std::string list = val("--mutscan_kinds");
            static const char *const names[5] = {"gain", "loss", "change", "same", "none"};
            x.mutscan_kinds = 0;
            for (size_t at = 0; at <= list.size();) {
                const size_t end = std::min(list.find(',', at), list.size());
                const std::string name = list.substr(at, end - at);
                int bit = -1;
                for (int q = 0; q < 5; q++)
                    if (name == names[q]) bit = q;
                if (bit < 0) {
                    fprintf(stderr, "error: --mutscan_kinds is a comma list of gain, loss, change, same, none\n");
                    return 2;
                }
                x.mutscan_kinds |= 1u << bit;
                at = end + 1;
            }
        }
        else if (k == "--affinity_output") x.affinity_output = val("--affinity_output");
        else if (k == "--affinity_mode") x.affinity_mode = mode_flag("--affinity_mode", val("--affinity_mode"), "all", TFBS_AFFINITY_ALL, "diff", TFBS_AFFINITY_DIFF);
        else if (k == "--affinity_rows_output") x.affinity_rows_output = val("--affinity_rows_output");
        else if (k == "--affinity_rows_min_spread") {
            char *end = nullptr;
            const char *v = val("--affinity_rows_min_spread");
            x.affinity_rows_min_spread = strtoull(v, &end, 10);
            if (end == v || *end || *v == '-') {
                fprintf(stderr, "error: --affinity_rows_min_spread is a count of milli-bits\n");
                return 2;
            }
        }
        else if (k == "--scores_output") x.scores_output = val("--scores_output");
        else if (k == "--scores_min_spread") x.scores_min_spread = strtoull(val("--scores_min_spread"), nullptr, 10);
        else if (k == "--pwm_pvalue") {
            char *end = nullptr;
            const char *v = val("--pwm_pvalue");
            x.pwm_pvalue = strtod(v, &end);
            if (end == v || *end || !(x.pwm_pvalue > 0) || !(x.pwm_pvalue < 1)) {
                fprintf(stderr, "error: --pwm_pvalue is a number above 0 and below 1\n");
                return 2;
            }
        }
        else if (k == "--pwm_threshold_directory") a.pwm_threshold_dir = val(k.c_str());
        else if (k == "--pwm_threshold" || k == "-t") {
            a.pwm_threshold = strtof(val(k.c_str()), nullptr);
            have_thr = true;
        } else if (k == "--forward_only" || k == "-f") a.forward_only = 1;
        else if (k == "--threads") {
            long n = strtol(val(k.c_str()), nullptr, 10);
            if (n < 1) {
                fprintf(stderr, "Wrong number of threads\n");
                return 2;
            }
            a.threads = (uint32_t)n;
        } else if (k == "--min_maf" || k == "-m") a.min_maf = (uint32_t)strtoul(val(k.c_str()), nullptr, 10);
        else if (k == "--after_position") a.after_position = strtoull(val(k.c_str()), nullptr, 10);
        else if (k == "--samples" || k == "-s") a.samples_file = val(k.c_str());
        else if (k == "--tabix" || k == "-z") a.tabix = 1;
        else if (k == "--verbose" || k == "-v") a.verbose = 1;
        else if (k == "--device") a.device = atoi(val(k.c_str()));
        else if (k == "--devices") a.devices = val(k.c_str());
        else if (k == "--gpus") {
            long n = strtol(val(k.c_str()), nullptr, 10);
            if (n < 1) {
                fprintf(stderr, "Wrong number of GPUs\n");
                return 2;
            }
            gpus.clear();
            for (long d = 0; d < n; d++) gpus += (d ? "," : "") + std::to_string(d);
            a.devices = gpus.c_str();
        }
        else if (k == "--regions_per_batch") a.regions_per_batch = (uint32_t)strtoul(val(k.c_str()), nullptr, 10);
        else if (k == "--help" || k == "-h") {
            usage();
            return 0;
        } else {
            fprintf(stderr, "error: unexpected argument '%s'\n", k.c_str());
            usage();
            return 2;
        }
    }
    if (!a.chromosome || !a.bcf || !a.output || !a.reference || !a.bed_files || !a.pwm_names ||
        (!a.pwm_file && !a.dipwm_file) || (!(x.pwm_pvalue > 0) && (!a.pwm_threshold_dir || !have_thr))) {
        usage();
        return 2;
    }
    int rc = tfbs_run_ex(&a, &x);
    if (rc) {
        fprintf(stderr, "find-tfbs-amd: %s (%s)\n", tfbs_last_error(), tfbs_strerror(rc));
        return 101;  // a Rust panic's exit status
    }
    printf("End of program.\n");
    return 0;
}
