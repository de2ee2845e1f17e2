// Dinucleotide tiles: pack TFBS_KIND_DIPWM strands (2 <= L <= 32 bases) into units
// of four interleaved k-mer lookup tables for scan_dinuc_kernel.
//
// A strand of L bases has R = L - 1 rows of 16 pair weights; the score of a window
// is the wrapping int32 sum of W[j][4 s[i+j] + s[i+j+1]] over its R transitions.
// Block b of a strand covers the transitions kDiStride b .. kDiStride b + kDiStride - 1
// (those below R): it maps the k-mer code of the bases kDiStride b .. kDiStride b + k - 1
// (first base in the low bits) to their sum, so consecutive blocks overlap by one base
// and a strand has ceil(R / kDiStride) blocks.  A transition at or past R adds nothing:
// the last block's entries do not depend on the bases past L.  Entries are wrapping
// int32, four strands interleaved per code (one 16-byte LDS read per lookup), like
// the LUT path's QUAD32 units.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "patterns.hpp"
#include "tfbs_internal.hpp"

namespace tfbs {

int check_dipwm_length(uint32_t L, const std::string &name) {
    if (L < 2)
        return fail(TFBS_E_ARG, "dinucleotide PWM '" + name + "' covers fewer than 2 bases (no row of 16 weights)");
    if (L > (uint32_t)kDiMaxLen)
        return fail(TFBS_E_ARG, "dinucleotide PWM '" + name + "' covers " + std::to_string(L) +
                                    " bases: more than the 32 the dinucleotide kernel scores");
    return TFBS_OK;
}

int check_kinds(const Patterns &P) {
    std::vector<uint8_t> seen(65536, 0);  // bit 0: a PWM strand, bit 1: a dinucleotide strand
    for (const Pat &p : P.pats) {
        if (p.kind != TFBS_KIND_PWM && p.kind != TFBS_KIND_DIPWM) continue;
        seen[p.pattern_id] |= p.kind == TFBS_KIND_PWM ? 1 : 2;
        if (seen[p.pattern_id] == 3)
            return fail(TFBS_E_ARG, "pattern_id " + std::to_string(p.pattern_id) +
                                        " mixes mononucleotide and dinucleotide strands");
    }
    return TFBS_OK;
}

namespace {

uint32_t di_blocks(uint32_t L) { return (L - 1 + kDiStride - 1) / kDiStride; }

// blocks of the units that `strands` (four to a unit, in order) make
uint32_t di_need(const Patterns &P, const std::vector<int> &strands) {
    uint32_t total = 0;
    for (size_t u = 0; u < strands.size(); u += 4) {
        uint32_t m = 0;
        for (size_t s = u; s < std::min(strands.size(), u + 4); s++) m = std::max(m, di_blocks(P.pats[strands[s]].len));
        total += m;
    }
    return total;
}

}  // namespace

int build_dinuc_tiles(const Patterns &P, const std::vector<SlotGroup> &groups, Plan *plan) {
    const uint32_t tile_blocks = kDiTileBytes / kDiBlockBytes;
    std::vector<int> cur;
    std::vector<uint32_t> cur_slot;
    uint32_t slot_begin = 0;
    auto close_tile = [&]() {
        if (cur.empty()) return;
        DevTile t{};
        t.first = (uint32_t)plan->di_units.size();
        t.lut_begin = (uint32_t)(plan->di_lut.size() / kDiBlockInts);
        t.slot_begin = slot_begin;
        t.lmin = UINT32_MAX;
        for (size_t u0 = 0; u0 < cur.size(); u0 += 4) {
            DevUnit U{};
            U.kind = UNIT_DINUC;
            U.lut_off = (uint32_t)(plan->di_lut.size() / kDiBlockInts) - t.lut_begin;
            const size_t n = std::min<size_t>(4, cur.size() - u0);
            U.nstrand = (uint32_t)n;
            for (size_t s = 0; s < (size_t)kUnitMax; s++) {
                if (s < n) {
                    const int i = cur[u0 + s];
                    const Pat &p = P.pats[i];
                    U.nblk = std::max(U.nblk, di_blocks(p.len));
                    U.thr[s] = p.min_score;
                    U.min_score[s] = p.min_score;
                    U.len[s] = p.len;
                    U.slot_local[s] = cur_slot[u0 + s] - slot_begin;
                    U.orig_index[s] = (uint32_t)i;
                    U.wofs[s] = (uint32_t)(plan->di_w.size() / 16);  // first row
                    plan->di_w.insert(plan->di_w.end(), p.w16.begin(), p.w16.end());
                    t.lmin = std::min(t.lmin, p.len);
                    plan->n_di_strands++;
                } else {  // padding strand: never matches
                    U.thr[s] = INT32_MAX;
                    U.min_score[s] = INT32_MAX;
                    U.len[s] = 0;
                    U.slot_local[s] = 0;
                    U.orig_index[s] = 0xFFFFFFFFu;
                    U.wofs[s] = 0;
                }
            }
            for (uint32_t b = 0; b < U.nblk; b++)
                for (uint32_t code = 0; code < (uint32_t)kDiCodes; code++)
                    for (size_t s = 0; s < 4; s++) {
                        uint32_t v = 0;
                        if (s < n) {
                            const Pat &p = P.pats[cur[u0 + s]];
                            for (uint32_t tr = 0; tr < (uint32_t)kDiStride; tr++) {
                                const uint32_t j = kDiStride * b + tr;  // transition: bases j, j + 1
                                if (j + 1 >= p.len) break;
                                const uint32_t pair = 4 * ((code >> (2 * tr)) & 3u) + ((code >> (2 * tr + 2)) & 3u);
                                v += (uint32_t)p.w16[16 * (size_t)j + pair];
                            }
                        }
                        plan->di_lut.push_back((int32_t)v);
                    }
            plan->di_units.push_back(U);
        }
        t.last = (uint32_t)plan->di_units.size();
        t.nblocks = (uint32_t)(plan->di_lut.size() / kDiBlockInts) - t.lut_begin;
        t.nslots = cur_slot.back() - slot_begin + 1;
        plan->max_di_tile_blocks = std::max(plan->max_di_tile_blocks, t.nblocks);
        plan->di_tiles.push_back(t);
        cur.clear();
        cur_slot.clear();
    };
    for (const SlotGroup &g0 : groups) {
        // a pattern_id's strands longest first: its units then need the fewest blocks (strands of
        // 4, 4, 7, 31 and 32 bases: 32 31 7 4 | 4, not 4 4 7 31 | 32 -- twice the blocks)
        SlotGroup g = g0;
        std::stable_sort(g.strands.begin(), g.strands.end(),
                         [&](int a, int b) { return P.pats[a].len > P.pats[b].len; });
        if (di_need(P, g.strands) > tile_blocks)
            return fail(TFBS_E_ARG, "the dinucleotide strands of pattern_id " +
                                        std::to_string(P.pats[g.strands[0]].pattern_id) +
                                        " exceed one tile's lookup tables (" + std::to_string(kDiTileBytes / 1024) +
                                        " KiB)");
        if (!cur.empty()) {
            std::vector<int> trial = cur;
            trial.insert(trial.end(), g.strands.begin(), g.strands.end());
            if (di_need(P, trial) > tile_blocks || g.slot - slot_begin + 1 > (uint32_t)kMaxTileSlots) close_tile();
        }
        if (cur.empty()) slot_begin = g.slot;
        for (int i : g.strands) {
            cur.push_back(i);
            cur_slot.push_back(g.slot);
        }
    }
    close_tile();
    return TFBS_OK;
}

// scan_dinuc.hip's lookup loop (di_chunks) on the host, from the arrays the upload
// copies: the 64-bit image with the first base in the low bits, per block the code
// (img >> (2 kDiStride b)) & (kDiCodes - 1), the strand's lane of the 16-byte entry and
// the wrapping sum over the unit's nblk blocks.  The rows (w16, di_w) are never read.
int dinuc_lut_scores(const Plan &plan, uint32_t pattern_index, const uint8_t *images, size_t n_images,
                     int32_t *out_scores) {
    for (const DevTile &t : plan.di_tiles)
        for (uint32_t ui = t.first; ui < t.last; ui++) {
            const DevUnit &U = plan.di_units[ui];
            for (uint32_t s = 0; s < U.nstrand; s++) {
                if (U.orig_index[s] != pattern_index) continue;
                const int32_t *base = plan.di_lut.data() + (size_t)(t.lut_begin + U.lut_off) * kDiBlockInts;
                for (size_t n = 0; n < n_images; n++) {
                    uint64_t img = 0;
                    for (int j = 0; j < kDiMaxLen; j++) {
                        const uint8_t c = images[(size_t)kDiMaxLen * n + j];
                        if (c > 3) return fail(TFBS_E_ARG, "image base code above 3");
                        img |= (uint64_t)c << (2 * j);
                    }
                    uint32_t sum = 0;
                    for (uint32_t b = 0; b < U.nblk; b++) {
                        const uint32_t code = (uint32_t)(img >> (2 * kDiStride * b)) & (uint32_t)(kDiCodes - 1);
                        sum += (uint32_t)base[(size_t)b * kDiBlockInts + 4 * code + s];
                    }
                    out_scores[n] = (int32_t)sum;
                }
                return TFBS_OK;
            }
        }
    return fail(TFBS_E_ARG, "pattern " + std::to_string(pattern_index) + " is not a dinucleotide strand of the plan");
}

}  // namespace tfbs
