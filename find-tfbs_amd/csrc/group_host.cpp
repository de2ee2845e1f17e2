// The grouping of build_gpu.hip in plain C++ (a DevGrouper in host memory), and the
// handle that drives a grouper alone (tfbs_grouper_*, include/tfbs_amd.h).
//
// The host grouper computes what the kernels compute -- every haplotype id's diff
// mask, the distinct masks in Vec<Diff> order with their carrier counts, one u16 of
// membership per id, overflow beyond kGrpMax masks -- with the same row stride, so a
// batch built through it (tfbs_batch_set_build_device(b, TFBS_GROUPER_HOST)) runs
// batch.cpp's device path (snv_prepare / mask_prepare, the chunk loop, snv_finish /
// mask_finish, the fetches) without a device.  Its device() is -1: the scan and the
// aggregation fetch its rows instead of reading them in place.
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "batch.hpp"

namespace tfbs {
namespace {

// Vec<Diff> order: the masks' ascending rank lists compared element by element
bool ranks_less(uint64_t a, uint64_t b) {
    uint8_t ra[64], rb[64];
    size_t na = 0, nb = 0;
    for (uint32_t k = 0; k < 64; k++) {
        if (a >> k & 1) ra[na++] = (uint8_t)k;
        if (b >> k & 1) rb[nb++] = (uint8_t)k;
    }
    return std::lexicographical_compare(ra, ra + na, rb, rb + nb);
}

struct HostGrouper final : DevGrouper {
    std::vector<uint32_t> car;
    std::vector<uint64_t> sig;  // one region's masks, zero between regions
    std::mutex memb_mu;
    std::vector<std::pair<uint16_t *, size_t>> memb_all, memb_free;  // as GpuGrouper's (u16 entries)

    ~HostGrouper() override {
        for (auto &m : memb_all) delete[] m.first;
    }
    int device() const override { return -1; }
    uint32_t *carriers(size_t n) override {
        car.resize(std::max<size_t>(n, 1));
        return car.data();
    }
    void recycle(std::vector<void *> &allocs) override {
        std::lock_guard<std::mutex> g(memb_mu);
        for (void *p : allocs)
            for (auto &m : memb_all)
                if (m.first == p) memb_free.push_back(m);
        allocs.clear();
    }
    uint16_t *memb_alloc(size_t n) {  // the smallest returned allocation that fits, else a new one
        std::lock_guard<std::mutex> g(memb_mu);
        size_t best = memb_free.size();
        for (size_t i = 0; i < memb_free.size(); i++)
            if (memb_free[i].second >= n && (best == memb_free.size() || memb_free[i].second < memb_free[best].second))
                best = i;
        if (best < memb_free.size()) {
            uint16_t *p = memb_free[best].first;
            memb_free.erase(memb_free.begin() + best);
            return p;
        }
        uint16_t *p = new (std::nothrow) uint16_t[n];
        if (p) memb_all.push_back({p, n});
        return p;
    }
    int group(size_t n_car, const std::vector<GrpRecord> &rv, const std::vector<GrpRegion> &rg, uint32_t H,
              GroupOut &out) override {
        const size_t nr = rg.size();
        out.n_groups.assign(nr, 0);
        out.first.assign(nr, 0);
        out.memb.assign(nr, 0);
        out.masks.clear();
        out.counts.clear();
        if (!nr) return TFBS_OK;
        const size_t stride = ((size_t)H + 7) / 8 * 8;  // GpuGrouper's rows
        uint16_t *mb = memb_alloc(std::max<size_t>(nr * stride, 8));
        if (!mb) return fail(TFBS_E_NOMEM, "host grouping: membership rows");
        out.memb_alloc = mb;
        sig.assign(H, 0);
        std::vector<uint32_t> ids;  // the region's ids with a mask, each once
        std::vector<uint64_t> distinct;
        std::unordered_map<uint64_t, uint32_t> at;  // mask -> carriers, then -> its index
        for (size_t j = 0; j < nr; j++) {
            uint16_t *row = mb + j * stride;
            out.memb[j] = (uint64_t)(uintptr_t)row;
            ids.clear();
            for (uint32_t q = 0; q < rg[j].n_rec; q++) {
                const GrpRecord &r = rv[rg[j].rec_off + q];
                for (uint32_t i = 0; i < r.n; i++) {
                    const uint32_t h = car[r.off + i];
                    if (!sig[h]) ids.push_back(h);
                    sig[h] |= 1ull << r.rank;
                }
            }
            at.clear();
            for (uint32_t h : ids) at[sig[h]]++;
            const size_t G = at.size();
            if (G > kGrpMax) {
                out.n_groups[j] = UINT32_MAX;
            } else {
                distinct.clear();
                for (auto &kv : at) distinct.push_back(kv.first);
                std::sort(distinct.begin(), distinct.end(), ranks_less);
                out.n_groups[j] = (uint32_t)G;
                out.first[j] = (uint32_t)out.masks.size();
                for (size_t i = 0; i < G; i++) {
                    uint32_t &v = at[distinct[i]];
                    out.masks.push_back(distinct[i]);
                    out.counts.push_back(v);
                    v = (uint32_t)i;
                }
                std::fill(row, row + H, (uint16_t)G);
                for (uint32_t h : ids) row[h] = (uint16_t)at[sig[h]];
            }
            for (uint32_t h : ids) sig[h] = 0;
        }
        return TFBS_OK;
    }
    int fetch(uint64_t m, uint32_t H, uint16_t *out) override {
        memcpy(out, (const void *)(uintptr_t)m, (size_t)H * 2);
        return TFBS_OK;
    }
};

}  // namespace

DevGrouper *make_host_grouper() { return new HostGrouper(); }

}  // namespace tfbs

struct tfbs_grouper {
    std::unique_ptr<tfbs::DevGrouper> g;
};

extern "C" {

int tfbs_grouper_create(int device, tfbs_grouper **out) {
    if (!out) return tfbs::fail(TFBS_E_ARG, "null argument");
    tfbs::DevGrouper *g = nullptr;
    if (device == TFBS_GROUPER_HOST) g = tfbs::make_host_grouper();
    else if (device >= 0) g = tfbs::make_gpu_grouper(device);
    else return tfbs::fail(TFBS_E_ARG, "a device index or TFBS_GROUPER_HOST");
    if (!g) return TFBS_E_NODEVICE;
    *out = new tfbs_grouper{std::unique_ptr<tfbs::DevGrouper>(g)};
    return TFBS_OK;
}

void tfbs_grouper_destroy(tfbs_grouper *g) { delete g; }

int tfbs_grouper_group(tfbs_grouper *g, uint32_t H, size_t n_regions, const uint32_t *n_records,
                       const uint32_t *n_carriers, const uint32_t *ids, uint32_t *n_groups, uint64_t *masks,
                       uint32_t *counts, size_t cap, size_t *n_masks, uint16_t *rows) {
    using namespace tfbs;
    if (!g || !n_masks || (n_regions && (!n_records || !n_groups || !rows))) return fail(TFBS_E_ARG, "null argument");
    *n_masks = 0;
    if (H == 0) return fail(TFBS_E_ARG, "no haplotype id");
    // one call is one launch: build_regions' chunk rule (batch.cpp)
    if (n_regions > 1024 || (uint64_t)n_regions * H > (1ull << 27))
        return fail(TFBS_E_ARG, "more regions than a chunk holds");
    std::vector<GrpRecord> recs;
    std::vector<GrpRegion> regs;
    uint64_t n_car = 0;
    size_t nrec = 0;
    for (size_t j = 0; j < n_regions; j++) {
        if (n_records[j] > 64) return fail(TFBS_E_ARG, "more than 64 records in a region");
        regs.push_back({(uint32_t)nrec, n_records[j]});
        if (n_records[j] && !n_carriers) return fail(TFBS_E_ARG, "null argument");
        for (uint32_t q = 0; q < n_records[j]; q++, nrec++) {
            const uint32_t n = n_carriers[nrec];
            if (n == 0) return fail(TFBS_E_ARG, "a record without a carrier");
            if (n > H || !ids) return fail(TFBS_E_ARG, "a record's carrier list");
            for (uint32_t i = 0; i < n; i++) {
                if (ids[n_car + i] >= H) return fail(TFBS_E_ARG, "carrier id beyond the haplotype ids");
                if (i && ids[n_car + i] <= ids[n_car + i - 1]) return fail(TFBS_E_ARG, "carrier ids not strictly ascending");
            }
            recs.push_back({(uint32_t)n_car, n, q, (uint32_t)j});
            n_car += n;
            if (n_car > (1ull << 30)) return fail(TFBS_E_ARG, "more carriers than a chunk holds");
        }
    }
    uint32_t *car = g->g->carriers((size_t)n_car);
    if (!car) return fail(TFBS_E_NOMEM, "grouping staging");
    if (n_car) memcpy(car, ids, (size_t)n_car * 4);
    GroupOut go;
    if (int rc = g->g->group((size_t)n_car, recs, regs, H, go)) return rc;
    std::vector<void *> allocs;
    if (go.memb_alloc) allocs.push_back(go.memb_alloc);
    int rc = TFBS_OK;
    size_t total = 0;
    for (size_t j = 0; j < n_regions; j++)
        if (go.n_groups[j] != UINT32_MAX) total += go.n_groups[j];
    *n_masks = total;
    if (total > cap || (total && (!masks || !counts))) rc = fail(TFBS_E_ARG, "output capacity too small");
    size_t at = 0;
    for (size_t j = 0; j < n_regions && !rc; j++) {
        n_groups[j] = go.n_groups[j];
        uint16_t *row = rows + j * (size_t)H;
        if (go.n_groups[j] == UINT32_MAX) {  // (the grouper leaves an overflowing region's row unwritten)
            std::fill(row, row + H, (uint16_t)0xFFFF);
            continue;
        }
        const uint32_t G = go.n_groups[j];
        if (G) {
            memcpy(masks + at, go.masks.data() + go.first[j], (size_t)G * 8);
            memcpy(counts + at, go.counts.data() + go.first[j], (size_t)G * 4);
        }
        at += G;
        rc = g->g->fetch(go.memb[j], H, row);
    }
    g->g->recycle(allocs);  // the rows go back to the grouper: the next call reuses them
    return rc;
}

}  // extern "C"
