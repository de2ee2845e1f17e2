// Pattern parsing and the device pattern plan.
//
// Parsing restates pattern.rs:13-112 (parse_weight, parse_threshold_file,
// parse_pwm_files, parse_pwm_definition, reverse_complement).  The plan turns
// the pattern list into what the scan kernels consume: pattern_id slots, tiles
// of strands whose 4-mer lookup tables fit the LDS budget, the tables
// themselves and the per-column A weights used for N correction.
// Dinucleotide PWMs (TFBS_KIND_DIPWM; no counterpart in the reference) parse
// from a second file of 16-column rows and plan into plan_dinuc.cpp's tiles.
#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "patterns.hpp"
#include "score_dist.hpp"
#include "tfbs_internal.hpp"

namespace tfbs {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

// Rust f32::from_str accepts [+-]digits[.digits][(e|E)[+-]digits], ".5", "5.",
// and inf/infinity/nan in any case; nothing else (no hex, no spaces).
static bool parse_f32_rust(const std::string &s, float *out) {
    size_t i = 0;
    if (i < s.size() && (s[i] == '+' || s[i] == '-')) i++;
    std::string rest = s.substr(i);
    std::string low;
    for (char c : rest) low.push_back((char)std::tolower((unsigned char)c));
    if (low == "inf" || low == "infinity" || low == "nan") {
        *out = std::strtof(s.c_str(), nullptr);
        return true;
    }
    size_t digits = 0;
    while (i < s.size() && std::isdigit((unsigned char)s[i])) { i++; digits++; }
    if (i < s.size() && s[i] == '.') {
        i++;
        while (i < s.size() && std::isdigit((unsigned char)s[i])) { i++; digits++; }
    }
    if (!digits) return false;
    if (i < s.size() && (s[i] == 'e' || s[i] == 'E')) {
        i++;
        if (i < s.size() && (s[i] == '+' || s[i] == '-')) i++;
        if (i >= s.size() || !std::isdigit((unsigned char)s[i])) return false;
        while (i < s.size() && std::isdigit((unsigned char)s[i])) i++;
    }
    if (i != s.size()) return false;
    *out = std::strtof(s.c_str(), nullptr);
    return true;
}

// pattern.rs:13-16.  The multiply is f32; round() is half away from zero; the
// `as i32` cast saturates and maps NaN to 0.
static int32_t milli(float x) {
    volatile float y = x * 1000.0f;
    float r = std::round((float)y);
    if (std::isnan(r)) return 0;
    if (r >= 2147483647.0f) return INT32_MAX;
    if (r <= -2147483648.0f) return INT32_MIN;
    return (int32_t)r;
}

static std::vector<std::string> split_ws(const std::string &line) {
    std::vector<std::string> out;
    std::istringstream is(line);
    std::string f;
    while (is >> f) out.push_back(f);
    return out;
}

int parse_weight(const std::string &s, int32_t *out) {
    float x;
    if (!parse_f32_rust(s, &x)) return fail(TFBS_E_PARSE, "cannot parse weight '" + s + "'");
    *out = milli(x);
    return TFBS_OK;
}

int parse_threshold_file(const std::string &path, float thr, int32_t *out) {
    std::ifstream in(path, std::ios::binary);
    if (!in) return fail(TFBS_E_IO, "Could not open file " + path);  // pattern.rs:116 expect
    std::string line;
    int found = 0;
    while (std::getline(in, line)) {
        auto f = split_ws(line);
        if (f.size() != 2) continue;
        int32_t w;
        float pv;
        int rc = parse_weight(f[0], &w);
        if (rc) return rc;
        if (!parse_f32_rust(f[1], &pv)) return fail(TFBS_E_PARSE, "Can't parse pvalue in file " + path);
        if (pv > thr) {  // the last qualifying line wins
            *out = w;
            found = 1;
        }
    }
    return found;
}

void Patterns::add(const Pat &p) {
    pats.push_back(p);
    names[p.pattern_id] = p.name;  // main.rs:239-250 HashMap insert: last wins
    slot_cache = std::make_shared<SlotCache>();  // (a copy keeps the old set's)
}

int Patterns::slot_order(std::vector<uint16_t> &slot_pid, bool &zero_len_panics) const {
    std::lock_guard<std::mutex> l(slot_cache->mu);
    SlotCache &c = *slot_cache;
    if (!c.built) {
        Plan plan;  // only its slot order is used (independent of the tile options)
        PlanOptions opt;
        opt.tile_blocks = 1u << 30;
        c.rc = build_plan(opt, &plan);
        c.slot_pid = std::move(plan.slot_pid);
        c.zero_len_panics = plan.zero_len_panics;
        c.built = true;
    }
    if (c.rc) return c.rc;
    slot_pid = c.slot_pid;
    zero_len_panics = c.zero_len_panics;
    return 0;
}

uint32_t Patterns::max_length() const {
    uint32_t m = 0;
    for (auto &p : pats) m = std::max<uint32_t>(m, p.kind == TFBS_KIND_PWM || p.kind == TFBS_KIND_DIPWM ? p.len : 0);
    return m;
}

static std::vector<int32_t> revcomp(const std::vector<int32_t> &w5, uint32_t L) {
    std::vector<int32_t> o(5 * (size_t)L);
    for (uint32_t j = 0; j < L; j++) {
        const int32_t *x = &w5[5 * (size_t)(L - 1 - j)];
        int32_t *y = &o[5 * (size_t)j];
        y[0] = x[3]; y[1] = x[2]; y[2] = x[1]; y[3] = x[0]; y[4] = 0;
    }
    return o;
}

// The reverse strand of a dinucleotide PWM: W'[i][4a + b] = W[R-1-i][4(3-b) + (3-a)],
// so its score on s is the forward strand's on the reverse complement of s.
static std::vector<int32_t> revcomp_di(const std::vector<int32_t> &w16) {
    const size_t R = w16.size() / 16;
    std::vector<int32_t> o(w16.size());
    for (size_t i = 0; i < R; i++)
        for (int a = 0; a < 4; a++)
            for (int b = 0; b < 4; b++) o[16 * i + 4 * a + b] = w16[16 * (R - 1 - i) + 4 * (3 - b) + (3 - a)];
    return o;
}

// One definitions file (pattern.rs:37-87): rows of ncol weights (4: a PWM, 16: a
// dinucleotide PWM), pattern ids from *next_id on.
int parse_definitions(const std::string &pwm_file, int ncol, const std::map<std::string, int32_t> &thresholds,
                      const std::vector<std::string> &wanted, bool add_reverse, uint16_t *next_id, Patterns *out) {
    std::ifstream in(pwm_file, std::ios::binary);
    if (!in) return fail(TFBS_E_IO, "Could not open file " + pwm_file);
    std::stringstream ss;
    ss << in.rdbuf();
    const std::string content = ss.str();
    uint16_t pattern_id = *next_id;
    size_t start = 0;
    while (start <= content.size()) {
        size_t gt = content.find('>', start);
        std::string chunk = content.substr(start, gt == std::string::npos ? std::string::npos : gt - start);
        start = gt == std::string::npos ? content.size() + 1 : gt + 1;
        if (chunk.empty()) continue;
        // parse_pwm_definition (pattern.rs:89-101)
        std::vector<std::string> lines;
        size_t a = 0;
        while (a <= chunk.size()) {
            size_t nl = chunk.find('\n', a);
            std::string l = chunk.substr(a, nl == std::string::npos ? std::string::npos : nl - a);
            if (!l.empty()) lines.push_back(l);
            if (nl == std::string::npos) break;
            a = nl + 1;
        }
        if (lines.empty()) return fail(TFBS_E_PARSE, "empty PWM definition");
        const std::string name = lines[0];
        std::vector<int32_t> w5, w16;
        for (size_t i = 1; i < lines.size(); i++) {
            auto f = split_ws(lines[i]);
            if (f.size() != (size_t)ncol) continue;
            int32_t v[16];
            for (int k = 0; k < ncol; k++) {
                int rc = parse_weight(f[k], &v[k]);
                if (rc) return rc;
            }
            if (ncol == 4) w5.insert(w5.end(), {v[0], v[1], v[2], v[3], 0});
            else w16.insert(w16.end(), v, v + 16);
        }
        if (std::find(wanted.begin(), wanted.end(), name) == wanted.end()) continue;
        auto it = thresholds.find(name);
        if (it != thresholds.end() && ncol == 16) {
            Pat p;
            p.kind = TFBS_KIND_DIPWM;
            p.direction = TFBS_DIR_P;
            p.pattern_id = pattern_id;
            p.min_score = it->second;
            p.len = (uint32_t)(w16.size() / 16) + 1;  // bases
            int rc = check_dipwm_length(p.len, name);
            if (rc) return rc;
            p.w16 = w16;
            p.name = name;
            out->add(p);
            if (add_reverse) {
                p.direction = TFBS_DIR_N;
                p.w16 = revcomp_di(w16);
                out->add(p);
            }
        } else if (it != thresholds.end()) {
            Pat p;
            p.kind = TFBS_KIND_PWM;
            p.direction = TFBS_DIR_P;
            p.pattern_id = pattern_id;
            p.min_score = it->second;
            p.len = (uint32_t)(w5.size() / 5);
            p.w5 = w5;
            p.name = name;
            out->add(p);
            if (add_reverse) {
                p.direction = TFBS_DIR_N;
                p.w5 = revcomp(w5, p.len);
                out->add(p);
            }
        }
        pattern_id = (uint16_t)(pattern_id + 1);  // pattern.rs:81
    }
    *next_id = pattern_id;
    return TFBS_OK;
}

int parse_pwm_files_di(const std::string *pwm_file, const std::string *dipwm_file, const std::string &thr_dir,
                       float thr, const std::vector<std::string> &wanted, bool add_reverse, Patterns *out) {
    std::map<std::string, int32_t> thresholds;
    std::string dir = thr_dir;
    while (!dir.empty() && dir.back() == '/') dir.pop_back();
    for (auto &name : wanted) {
        int32_t v;
        int r = parse_threshold_file(dir + "/" + name + ".thr", thr, &v);
        if (r < 0) return r;
        if (r == 1) thresholds[name] = v;
    }
    uint16_t next_id = 0;
    int rc = 0;
    if (pwm_file) rc = parse_definitions(*pwm_file, 4, thresholds, wanted, add_reverse, &next_id, out);
    if (!rc && dipwm_file) rc = parse_definitions(*dipwm_file, 16, thresholds, wanted, add_reverse, &next_id, out);
    if (rc) return rc;
    if (out->pats.empty()) return fail(TFBS_E_NOPATTERN, "no pattern loaded");  // main.rs:238
    return TFBS_OK;
}

int parse_pwm_files(const std::string &pwm_file, const std::string &thr_dir, float thr,
                    const std::vector<std::string> &wanted, bool add_reverse, Patterns *out) {
    return parse_pwm_files_di(&pwm_file, nullptr, thr_dir, thr, wanted, add_reverse, out);
}

// ---------------------------------------------------------------------------
// Device plan
// ---------------------------------------------------------------------------
struct Group { uint16_t pid; bool generic; uint32_t maxlen; std::vector<int> strands; };
static std::vector<SlotGroup> groups_fast(const std::vector<Group> &groups) {
    std::vector<SlotGroup> out;
    for (uint32_t gi = 0; gi < groups.size(); gi++)
        if (!groups[gi].generic) out.push_back({gi, groups[gi].strands});
    return out;
}
// Strands are grouped by pattern_id (both strands of a PWM share it and their
// hits add into one count, main.rs:505).  Groups are ordered by (needs the
// generic kernel, longest strand, pattern_id) -- this order defines the count
// slots -- so neighbouring strands have similar lengths and pack into units
// with little padding.  Fast tiles are runs of whole groups whose table blocks
// fit the LDS budget and span at most 64 slots.
// With opt.mfma, groups whose strands all pass mfma_eligible are scored on the
// matrix cores instead (32-strand tiles, any slot mix: that kernel adds its
// counts atomically).
int Patterns::build_plan(const PlanOptions &opt, Plan *plan) const {
    *plan = Plan();
    // Scannable strands: PWM with length >= 1.  A length-0 PWM with a negative
    // min_score panics in the reference at the first region (pattern.rs:150-156
    // reads haplotype[len]); with min_score >= 0 it never matches.
    std::map<uint16_t, std::vector<int>> by_pid, di_by_pid;
    if (int rc = check_kinds(*this)) return rc;
    for (size_t i = 0; i < pats.size(); i++) {
        const Pat &p = pats[i];
        if (p.kind == TFBS_KIND_DIPWM) {
            if (int rc = check_dipwm_length(p.len, p.name)) return rc;
            di_by_pid[p.pattern_id].push_back((int)i);
        }
        if (p.kind != TFBS_KIND_PWM) continue;
        if (p.len == 0) {
            if (p.min_score < 0) plan->zero_len_panics = true;
            continue;
        }
        by_pid[p.pattern_id].push_back((int)i);
    }
    if (pats.size() > 65535) return fail(TFBS_E_ARG, "more than 65535 patterns");
    std::vector<Group> groups;
    for (auto &kv : by_pid) {
        Group g{kv.first, false, 0, kv.second};
        for (int i : g.strands) {
            g.maxlen = std::max(g.maxlen, pats[i].len);
            if (pats[i].len > (uint32_t)kFastMaxLen) g.generic = true;
        }
        groups.push_back(std::move(g));
    }
    std::stable_sort(groups.begin(), groups.end(), [](const Group &a, const Group &b) {
        if (a.generic != b.generic) return !a.generic;
        if (a.maxlen != b.maxlen) return a.maxlen < b.maxlen;
        return a.pid < b.pid;
    });
    for (auto &g : groups) plan->slot_pid.push_back(g.pid);
    std::vector<SlotGroup> fast = groups_fast(groups), lut, mat;
    for (SlotGroup &g : fast) {
        bool m = opt.mfma;
        for (int i : g.strands) m = m && mfma_eligible(pats[i]);
        (m ? mat : lut).push_back(std::move(g));
    }
    plan->slot_mfma.assign(groups.size(), 0);
    for (const SlotGroup &g : mat) plan->slot_mfma[g.slot] = 1;
    build_fast_tiles(*this, lut, opt.tile_blocks, plan);
    build_mfma_tiles(*this, mat, opt, plan);
    // --- generic (long) strands: one tile per pattern_id group, weights x5
    for (uint32_t gi = 0; gi < groups.size(); gi++) {
        const Group &g = groups[gi];
        if (!g.generic) continue;
        DevTile t{};
        t.first = (uint32_t)plan->gen_pats.size();
        t.slot_begin = gi;
        t.nslots = 1;
        t.lmin = UINT32_MAX;
        for (int i : g.strands) {
            const Pat &p = pats[i];
            if (p.len > 65535) return fail(TFBS_E_ARG, "pattern longer than 65535 columns");
            DevPattern d{};
            d.col_off = (uint32_t)(plan->gen_w.size() / 5);
            d.min_score = p.min_score;
            d.len = p.len;
            d.slot_local = 0;
            d.orig_index = (uint32_t)i;
            t.lmin = std::min<uint32_t>(t.lmin, p.len);
            plan->gen_pats.push_back(d);
            for (uint32_t j = 0; j < p.len; j++)
                for (int c = 0; c < 5; c++) plan->gen_w.push_back(c == 4 ? 0 : p.w5[5 * j + c]);
        }
        t.last = (uint32_t)plan->gen_pats.size();
        plan->gen_tiles.push_back(t);
    }
    for (auto &t : plan->fast_tiles) plan->max_tile_blocks = std::max(plan->max_tile_blocks, t.nblocks);
    // --- dinucleotide strands: slots after every other group's, ordered by (longest
    // strand, pattern_id); dense counts (slot_mfma 0), scored by scan_dinuc_kernel
    if (!di_by_pid.empty()) {
        std::vector<Group> dg;
        for (auto &kv : di_by_pid) {
            Group g{kv.first, false, 0, kv.second};
            for (int i : g.strands) g.maxlen = std::max(g.maxlen, pats[i].len);
            dg.push_back(std::move(g));
        }
        std::stable_sort(dg.begin(), dg.end(), [](const Group &a, const Group &b) {
            if (a.maxlen != b.maxlen) return a.maxlen < b.maxlen;
            return a.pid < b.pid;
        });
        std::vector<SlotGroup> di;
        for (auto &g : dg) {
            di.push_back({(uint32_t)plan->slot_pid.size(), g.strands});
            plan->slot_pid.push_back(g.pid);
            plan->slot_mfma.push_back(0);
        }
        if (int rc = build_dinuc_tiles(*this, di, plan)) return rc;
    }
    return TFBS_OK;
}

}  // namespace tfbs

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
using tfbs::Patterns;

extern "C" {

struct tfbs_patterns {
    Patterns p;
};

const char *tfbs_last_error(void) { return tfbs::g_last_error.c_str(); }

const char *tfbs_version(void) { return "find-tfbs_amd 0.2 (gfx950)"; }

const char *tfbs_strerror(int code) {
    switch (code) {
    case TFBS_OK: return "ok";
    case TFBS_E_ARG: return "bad argument";
    case TFBS_E_BADBASE: return "unknown nucleotide";
    case TFBS_E_REFMISMATCH: return "variant REF does not match the reference genome";
    case TFBS_E_MNP: return "missing case in haplotype patcher (MNP)";
    case TFBS_E_PLOIDY: return "inconsistent number of alleles";
    case TFBS_E_RANGE: return "region out of range";
    case TFBS_E_PARSE: return "parse error";
    case TFBS_E_IO: return "I/O error";
    case TFBS_E_HIP: return "HIP error";
    case TFBS_E_NODEVICE: return "no HIP device";
    case TFBS_E_ALLELES: return "record has a single allele";
    case TFBS_E_ZEROLEN: return "length-0 PWM with a negative min_score";
    case TFBS_E_NOPATTERN: return "no pattern";
    case TFBS_E_STATE: return "bad call order";
    case TFBS_E_NOMEM: return "out of memory";
    default: return "unknown error";
    }
}

int tfbs_parse_weight(const char *s, int32_t *out) {
    if (!s || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    return tfbs::parse_weight(s, out);
}

int tfbs_parse_threshold_file(const char *path, float thr, int32_t *out) {
    if (!path || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    return tfbs::parse_threshold_file(path, thr, out);
}

static std::vector<std::string> split_names(const char *names_csv) {
    std::vector<std::string> wanted;
    std::string s(names_csv);
    size_t a = 0;
    for (;;) {  // split(',') keeps empty pieces (main.rs:197)
        size_t c = s.find(',', a);
        wanted.push_back(s.substr(a, c == std::string::npos ? std::string::npos : c - a));
        if (c == std::string::npos) break;
        a = c + 1;
    }
    return wanted;
}

int tfbs_patterns_create(const tfbs_pattern_desc *d, size_t n, tfbs_patterns **out) {
    if (!out || (n && !d)) return tfbs::fail(TFBS_E_ARG, "null argument");
    auto *ps = new tfbs_patterns();
    for (size_t i = 0; i < n; i++) {
        tfbs::Pat p;
        p.kind = d[i].kind;
        p.direction = d[i].direction;
        p.pattern_id = d[i].pattern_id;
        p.min_score = d[i].min_score;
        p.len = d[i].kind == TFBS_KIND_PWM || d[i].kind == TFBS_KIND_DIPWM ? d[i].length : 0;
        p.name = d[i].name ? d[i].name : "";
        if (p.kind != TFBS_KIND_PWM && p.kind != TFBS_KIND_OTHER && p.kind != TFBS_KIND_DIPWM) {
            delete ps;
            return tfbs::fail(TFBS_E_ARG, "unknown pattern kind");
        }
        if (p.kind == TFBS_KIND_DIPWM) {  // length bases, (length - 1) x 16 pair weights
            int rc = tfbs::check_dipwm_length(p.len, p.name);
            if (!rc && !d[i].weights) rc = tfbs::fail(TFBS_E_ARG, "dinucleotide PWM without weights");
            if (rc) {
                delete ps;
                return rc;
            }
            p.w16.assign(d[i].weights, d[i].weights + 16 * (size_t)(p.len - 1));
            ps->p.add(p);
            continue;
        }
        if (p.len && !d[i].weights) {
            delete ps;
            return tfbs::fail(TFBS_E_ARG, "PWM without weights");
        }
        p.w5.resize(5 * (size_t)p.len);
        for (size_t j = 0; j < p.len; j++) {
            for (int c = 0; c < 4; c++) p.w5[5 * j + c] = d[i].weights[5 * j + c];
            p.w5[5 * j + 4] = 0;  // Weight::new forces N = 0 (types.rs:109-113)
        }
        ps->p.add(p);
    }
    if (int rc = tfbs::check_kinds(ps->p)) {
        delete ps;
        return rc;
    }
    *out = ps;
    return TFBS_OK;
}

int tfbs_patterns_from_files_di(const char *pwm_file, const char *dipwm_file, const char *thr_dir, float thr,
                                const char *names_csv, int add_reverse, tfbs_patterns **out) {
    if ((!pwm_file && !dipwm_file) || !thr_dir || !names_csv || !out)
        return tfbs::fail(TFBS_E_ARG, "null argument");
    const std::vector<std::string> wanted = split_names(names_csv);
    auto *ps = new tfbs_patterns();
    const std::string mono = pwm_file ? pwm_file : "", di = dipwm_file ? dipwm_file : "";
    int rc = tfbs::parse_pwm_files_di(pwm_file ? &mono : nullptr, dipwm_file ? &di : nullptr, thr_dir, thr, wanted,
                                      add_reverse != 0, &ps->p);
    if (!rc) rc = tfbs::check_kinds(ps->p);
    if (rc) {
        delete ps;
        return rc;
    }
    *out = ps;
    return TFBS_OK;
}

int tfbs_patterns_from_files(const char *pwm_file, const char *thr_dir, float thr, const char *names_csv,
                             int add_reverse, tfbs_patterns **out) {
    if (!pwm_file || !thr_dir || !names_csv || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    const std::vector<std::string> wanted = split_names(names_csv);
    auto *ps = new tfbs_patterns();
    int rc = tfbs::parse_pwm_files(pwm_file, thr_dir, thr, wanted, add_reverse != 0, &ps->p);
    if (rc) {
        delete ps;
        return rc;
    }
    *out = ps;
    return TFBS_OK;
}

int tfbs_patterns_with_min_scores(const tfbs_patterns *p, const int32_t *min_scores, tfbs_patterns **out) {
    if (!p || !out || (!min_scores && !p->p.pats.empty())) return tfbs::fail(TFBS_E_ARG, "null argument");
    auto *ps = new tfbs_patterns();
    for (size_t i = 0; i < p->p.pats.size(); i++) {  // (add: a slot cache of its own, the names as p made them)
        tfbs::Pat q = p->p.pats[i];
        q.min_score = min_scores[i];
        ps->p.add(q);
    }
    *out = ps;
    return TFBS_OK;
}

int tfbs_patterns_from_files_pvalue(const char *pwm_file, const char *dipwm_file, const char *names_csv,
                                    int add_reverse, int device, double pvalue, tfbs_patterns **out) {
    if ((!pwm_file && !dipwm_file) || !names_csv || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (int rc = tfbs::dist_check_pvalue(pvalue)) return rc;
    const std::vector<std::string> wanted = split_names(names_csv);
    std::map<std::string, int32_t> named;  // every named definition loads
    for (auto &name : wanted) named[name] = 0;
    tfbs_patterns loaded;
    uint16_t next_id = 0;
    int rc = 0;
    if (pwm_file) rc = tfbs::parse_definitions(pwm_file, 4, named, wanted, add_reverse != 0, &next_id, &loaded.p);
    if (!rc && dipwm_file)
        rc = tfbs::parse_definitions(dipwm_file, 16, named, wanted, add_reverse != 0, &next_id, &loaded.p);
    if (!rc && loaded.p.pats.empty()) rc = tfbs::fail(TFBS_E_NOPATTERN, "no pattern loaded");
    if (!rc) rc = tfbs::check_kinds(loaded.p);
    if (rc) return rc;
    std::vector<int32_t> ms(loaded.p.pats.size());
    if ((rc = tfbs::pvalue_thresholds(loaded.p, device, pvalue, ms.data()))) return rc;
    return tfbs_patterns_with_min_scores(&loaded, ms.data(), out);
}

size_t tfbs_patterns_count(const tfbs_patterns *p) { return p ? p->p.pats.size() : 0; }

int tfbs_patterns_get(const tfbs_patterns *p, size_t i, tfbs_pattern_desc *out) {
    if (!p || !out || i >= p->p.pats.size()) return tfbs::fail(TFBS_E_ARG, "bad pattern index");
    const tfbs::Pat &q = p->p.pats[i];
    out->pattern_id = q.pattern_id;
    out->direction = (uint8_t)q.direction;
    out->kind = (uint8_t)q.kind;
    out->length = q.len;
    out->weights = q.kind == TFBS_KIND_DIPWM ? q.w16.data() : q.w5.empty() ? nullptr : q.w5.data();
    out->min_score = q.min_score;
    out->name = q.name.c_str();
    return TFBS_OK;
}

const char *tfbs_patterns_name_of(const tfbs_patterns *p, uint16_t pid) {
    if (!p) return nullptr;
    auto it = p->p.names.find(pid);
    return it == p->p.names.end() ? nullptr : it->second.c_str();
}

uint32_t tfbs_patterns_max_length(const tfbs_patterns *p) { return p ? p->p.max_length() : 0; }

void tfbs_patterns_destroy(tfbs_patterns *p) { delete p; }

int tfbs_patterns_plan_stats(const tfbs_patterns *p, uint32_t tile_blocks, int mfma, tfbs_plan_stats *out) {
    if (!p || !out) return tfbs::fail(TFBS_E_ARG, "null argument");
    tfbs::Plan plan;
    tfbs::PlanOptions opt;
    opt.tile_blocks = tile_blocks;
    opt.mfma = mfma != 0;
    int rc = p->p.build_plan(opt, &plan);
    if (rc) return rc;
    *out = tfbs_plan_stats{};
    out->n_octet_strands = plan.n_octet_strands;
    out->n_quad_strands = plan.n_quad_strands;
    out->n_generic_strands = (uint32_t)plan.gen_pats.size();
    out->n_fast_tiles = (uint32_t)plan.fast_tiles.size();
    out->n_fast_units = (uint32_t)plan.fast_units.size();
    out->n_generic_tiles = (uint32_t)plan.gen_tiles.size();
    out->max_tile_blocks = plan.max_tile_blocks;
    out->lut_bytes = (uint64_t)plan.lut.size() * 4;
    out->n_mfma_strands = plan.n_mfma_strands;
    out->n_mfma_tiles = plan.n_mfma_tiles;
    out->n_mfma_supers = (uint32_t)plan.m_supers.size();
    return TFBS_OK;
}

int tfbs_patterns_dinuc_stats(const tfbs_patterns *p, uint32_t *n_strands, uint32_t *n_tiles, uint64_t *lut_bytes) {
    if (!p) return tfbs::fail(TFBS_E_ARG, "null argument");
    tfbs::Plan plan;
    tfbs::PlanOptions opt;
    int rc = p->p.build_plan(opt, &plan);
    if (rc) return rc;
    if (n_strands) *n_strands = plan.n_di_strands;
    if (n_tiles) *n_tiles = (uint32_t)plan.di_tiles.size();
    if (lut_bytes) *lut_bytes = (uint64_t)plan.di_lut.size() * 4;
    return TFBS_OK;
}

int tfbs_patterns_dinuc_lut_scores(const tfbs_patterns *p, size_t i, const uint8_t *images, size_t n_images,
                                   int32_t *out_scores) {
    if (!p || (n_images && (!images || !out_scores))) return tfbs::fail(TFBS_E_ARG, "null argument");
    if (i >= p->p.pats.size() || p->p.pats[i].kind != TFBS_KIND_DIPWM)
        return tfbs::fail(TFBS_E_ARG, "not the index of a dinucleotide strand");
    tfbs::Plan plan;
    tfbs::PlanOptions opt;
    int rc = p->p.build_plan(opt, &plan);
    if (rc) return rc;
    return tfbs::dinuc_lut_scores(plan, (uint32_t)i, images, n_images, out_scores);
}

int tfbs_patterns_mfma_bound(const tfbs_patterns *p, size_t i, const uint8_t *bases, tfbs_mfma_bound *out) {
    if (!p || !out || (!bases && i < p->p.pats.size() && p->p.pats[i].len))
        return tfbs::fail(TFBS_E_ARG, "null argument");
    if (i >= p->p.pats.size()) return tfbs::fail(TFBS_E_ARG, "pattern index out of range");
    const tfbs::Pat &pat = p->p.pats[i];
    *out = tfbs_mfma_bound{};
    for (uint32_t j = 0; j < pat.len; j++)
        if (bases[j] > 4) return tfbs::fail(TFBS_E_ARG, "base code above 4");
    if (!tfbs::mfma_eligible(pat)) return TFBS_OK;
    out->eligible = 1;
    tfbs::mfma_window_bound(pat, bases, &out->q8, &out->t8, &out->scale, &out->c);
    return TFBS_OK;
}

int tfbs_patterns_mfma_plan(const tfbs_patterns *p, uint32_t lds_kb, uint8_t *image, size_t image_cap,
                            size_t *image_bytes, tfbs_mfma_super *supers, size_t supers_cap, size_t *n_supers,
                            int32_t *meta, size_t meta_cap, size_t *meta_ints) {
    if (!p || !image_bytes || !n_supers || !meta_ints) return tfbs::fail(TFBS_E_ARG, "null argument");
    tfbs::Plan plan;
    tfbs::PlanOptions opt;  // as tfbs_ctx_create sets them (TFBS_MFMA=1, TFBS_MFMA_LDS_KB=lds_kb)
    opt.mfma = true;
    opt.mfma_lds_bytes = std::min<uint32_t>(144, std::max<uint32_t>(8, lds_kb ? lds_kb : 44)) * 1024u;
    int rc = p->p.build_plan(opt, &plan);
    if (rc) return rc;
    *image_bytes = plan.m_image.size() * 4;
    *n_supers = plan.m_supers.size();
    *meta_ints = plan.m_meta.size();
    if ((image && image_cap < *image_bytes) || (supers && supers_cap < *n_supers) || (meta && meta_cap < *meta_ints))
        return tfbs::fail(TFBS_E_ARG, "output capacity too small");
    if (image && *image_bytes) std::memcpy(image, plan.m_image.data(), *image_bytes);
    if (meta && *meta_ints) std::memcpy(meta, plan.m_meta.data(), *meta_ints * 4);
    if (supers)
        for (size_t k = 0; k < plan.m_supers.size(); k++) {
            const tfbs::DevMSuper &S = plan.m_supers[k];
            supers[k] = tfbs_mfma_super{S.tile_count, S.nk, S.img_off, S.img_bytes, S.seg, S.t0, S.acc0, S.lmin,
                                        S.lmax, S.tile0};
        }
    return TFBS_OK;
}

int tfbs_patterns_lut_plan(const tfbs_patterns *p, uint32_t tile_blocks, int mfma, const tfbs_lut_plan_buffers *buf,
                           tfbs_lut_plan_sizes *sizes) {
    if (!p || !sizes) return tfbs::fail(TFBS_E_ARG, "null argument");
    tfbs::Plan plan;
    tfbs::PlanOptions opt;
    opt.tile_blocks = tile_blocks;
    opt.mfma = mfma != 0;
    int rc = p->p.build_plan(opt, &plan);
    if (rc) return rc;
    const size_t n_slots = plan.slot_pid.size();  // (a set's dinucleotide slots come last)
    *sizes = tfbs_lut_plan_sizes{plan.fast_tiles.size(), plan.fast_units.size(), plan.lut.size(),
                                 plan.gen_tiles.size(),  plan.gen_pats.size(),   plan.gen_w.size(), n_slots};
    if (!buf) return TFBS_OK;
    if ((buf->tiles && buf->tiles_cap < sizes->n_tiles) || (buf->units && buf->units_cap < sizes->n_units) ||
        (buf->lut && buf->lut_cap < sizes->lut_ints) || (buf->gen_tiles && buf->gen_tiles_cap < sizes->n_gen_tiles) ||
        (buf->gen_pats && buf->gen_pats_cap < sizes->n_gen_pats) || (buf->gen_w && buf->gen_w_cap < sizes->gen_w_ints) ||
        (buf->slot_pid && buf->slot_pid_cap < n_slots) || (buf->slot_mfma && buf->slot_mfma_cap < n_slots))
        return tfbs::fail(TFBS_E_ARG, "output capacity too small");
    auto tile = [](const tfbs::DevTile &t) {
        return tfbs_lut_tile{t.first, t.last, t.lut_begin, t.nblocks, t.slot_begin, t.nslots, t.lmin};
    };
    if (buf->tiles)
        for (size_t k = 0; k < plan.fast_tiles.size(); k++) buf->tiles[k] = tile(plan.fast_tiles[k]);
    if (buf->gen_tiles)
        for (size_t k = 0; k < plan.gen_tiles.size(); k++) buf->gen_tiles[k] = tile(plan.gen_tiles[k]);
    if (buf->units)
        for (size_t k = 0; k < plan.fast_units.size(); k++) {
            const tfbs::DevUnit &U = plan.fast_units[k];
            tfbs_lut_unit &o = buf->units[k];
            o.lut_off = U.lut_off;
            o.nblk = U.nblk;
            o.nstrand = U.nstrand;
            o.kind = U.kind;
            std::copy(U.init, U.init + 4, o.init);
            std::copy(U.thr, U.thr + 8, o.thr);
            std::copy(U.min_score, U.min_score + 8, o.min_score);
            std::copy(U.len, U.len + 8, o.len);
            std::copy(U.slot_local, U.slot_local + 8, o.slot_local);
            std::copy(U.orig_index, U.orig_index + 8, o.orig_index);
        }
    if (buf->gen_pats)
        for (size_t k = 0; k < plan.gen_pats.size(); k++) {
            const tfbs::DevPattern &d = plan.gen_pats[k];
            buf->gen_pats[k] = tfbs_lut_gen_pat{d.col_off, d.min_score, d.len, d.slot_local, d.orig_index};
        }
    if (buf->lut) std::copy(plan.lut.begin(), plan.lut.end(), buf->lut);
    if (buf->gen_w) std::copy(plan.gen_w.begin(), plan.gen_w.end(), buf->gen_w);
    if (buf->slot_pid) std::copy(plan.slot_pid.begin(), plan.slot_pid.begin() + n_slots, buf->slot_pid);
    if (buf->slot_mfma) std::copy(plan.slot_mfma.begin(), plan.slot_mfma.begin() + n_slots, buf->slot_mfma);
    return TFBS_OK;
}

}  // extern "C"

namespace tfbs {
const Patterns &patterns_of(const tfbs_patterns *p) { return p->p; }
}  // namespace tfbs
