// The run flow's ordering pieces (run.cpp), host-only: the POS chain that numbers the batches'
// rows across the devices' threads, the sequencer that writes the batches' texts in batch
// order, and the split of a batch into whole regions under a record limit.
#pragma once

#include <condition_variable>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/tfbs_amd.h"

namespace tfbs {

// Batch g's first POS is batch g - 1's plus its rows, published as soon as g - 1 has counted
// them.  mu / cv / failed are open to an owner that waits on more than the chain (Ordered).
struct PosChain {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<int64_t> base;  // POS of batch g's first row, -1 unknown
    bool failed = false;
    explicit PosChain(size_t n_batches) : base(n_batches + 1, -1) { base[0] = 1; }
    // waits for batch g's first POS (*fake), then publishes batch g + 1's; TFBS_E_STATE after abort()
    int chain(size_t g, uint64_t n_rows, uint32_t *fake) {
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return failed || base[g] >= 0; });
        if (failed) return TFBS_E_STATE;
        *fake = (uint32_t)base[g];
        base[g + 1] = base[g] + (int64_t)n_rows;
        cv.notify_all();
        return TFBS_OK;
    }
    void abort() {
        std::lock_guard<std::mutex> l(mu);
        failed = true;
        cv.notify_all();
    }
};

// Texts handed in by batch index in any order, from any thread, given to the sink in index
// order, each once.  The sink's first failure stops the writing: that submit and every later
// one return it.
template <class Sink>  // int(const char *, size_t)
struct InOrder {
    std::mutex mu;
    Sink sink;
    std::map<size_t, std::string> pending;  // batches past `next`, waiting for their turn
    size_t next = 0;
    int rc = TFBS_OK;
    explicit InOrder(Sink s) : sink(std::move(s)) {}
    int submit(size_t g, std::string &&text) {
        std::lock_guard<std::mutex> l(mu);
        pending[g] = std::move(text);
        for (auto it = pending.begin(); !rc && it != pending.end() && it->first == next; it = pending.erase(it), next++)
            rc = sink(it->second.data(), it->second.size());
        return rc;
    }
};

// fn(q0, q1) over consecutive slices of [0, n_regions): each as many whole regions as keep
// the sum of records_of <= limit, one region at least; stops at fn's first failure.
template <class RecordsOf, class Fn>
int for_whole_regions(size_t n_regions, RecordsOf &&records_of, size_t limit, Fn &&fn) {
    for (size_t q0 = 0; q0 < n_regions;) {
        size_t q1 = q0 + 1, recs = records_of(q0);
        while (q1 < n_regions && recs + records_of(q1) <= limit) recs += records_of(q1++);
        if (int rc = fn(q0, q1)) return rc;
        q0 = q1;
    }
    return TFBS_OK;
}

}  // namespace tfbs
