// The run flow's ordering pieces (find-tfbs_amd/csrc/run_order.hpp) alone, as a host program
// built with the thread sanitizer (tests/test_run_order_cpu.py): the in-order sequencer under
// eight submitting threads and a failing sink, the POS chain under eight chaining threads and
// an abort from outside, and the whole-region split at its edges.  Exit status 0: every check held.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <future>
#include <numeric>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../find-tfbs_amd/csrc/run_order.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                               \
        }                                                             \
    } while (0)

constexpr int kThreads = 8;
constexpr size_t kBatches = 200;

std::vector<size_t> shuffled(size_t n, unsigned seed) {
    std::vector<size_t> v(n);
    std::iota(v.begin(), v.end(), (size_t)0);
    std::shuffle(v.begin(), v.end(), std::mt19937(seed));
    return v;
}

// fn(g) for the shuffled indices, thread t taking every kThreads-th of them
template <class Fn>
void on_threads(const std::vector<size_t> &order, Fn fn) {
    std::vector<std::thread> ts;
    for (int t = 0; t < kThreads; t++)
        ts.emplace_back([&, t] {
            for (size_t i = (size_t)t; i < order.size(); i += kThreads) fn(order[i]);
        });
    for (auto &t : ts) t.join();
}

void sequencer_in_order() {
    std::vector<std::string> seen;  // (written by the sink alone: under the sequencer's mutex)
    auto sink = [&](const char *p, size_t n) {
        seen.emplace_back(p, n);
        return TFBS_OK;
    };
    tfbs::InOrder<decltype(sink)> seq(sink);
    std::atomic<int> bad(0);
    on_threads(shuffled(kBatches, 1), [&](size_t g) {
        if (seq.submit(g, "text " + std::to_string(g) + "\n") != TFBS_OK) bad++;
    });
    CHECK(bad == 0);
    CHECK(seen.size() == kBatches);
    for (size_t g = 0; g < seen.size(); g++) CHECK(seen[g] == "text " + std::to_string(g) + "\n");
    CHECK(seq.pending.empty() && seq.next == kBatches);
}

void sequencer_failing_sink() {
    constexpr size_t kFailAt = 57;
    std::vector<std::string> seen;
    size_t calls = 0;
    auto sink = [&](const char *p, size_t n) {
        if (calls++ == kFailAt) return TFBS_E_IO;
        seen.emplace_back(p, n);
        return TFBS_OK;
    };
    tfbs::InOrder<decltype(sink)> seq(sink);
    // the submit that reaches the failing write returns the error, and so does every submit after it
    std::mutex mu;
    bool failed = false;
    int late_ok = 0, errors = 0;
    on_threads(shuffled(kBatches, 2), [&](size_t g) {
        std::lock_guard<std::mutex> l(mu);  // (one submit at a time: "later" is well defined)
        const int rc = seq.submit(g, std::to_string(g));
        if (rc) {
            CHECK(rc == TFBS_E_IO);
            failed = true;
            errors++;
        } else if (failed) {
            late_ok++;
        }
    });
    CHECK(failed && late_ok == 0 && errors >= 1);
    CHECK(calls == kFailAt + 1);  // nothing is tried past the failure
    CHECK(seen.size() == kFailAt);
    for (size_t g = 0; g < seen.size(); g++) CHECK(seen[g] == std::to_string(g));
    CHECK(seq.submit(kBatches, "late") == TFBS_E_IO);
}

void chain_prefix_sums() {
    std::vector<uint64_t> rows(kBatches);
    std::mt19937 rng(3);
    for (auto &r : rows) r = rng() % 1000;  // (zeros among them)
    rows[5] = 0;
    std::vector<uint32_t> fake(kBatches, 0);
    std::atomic<int> bad(0);
    tfbs::PosChain chain(kBatches);
    // a thread takes its indices in ascending order, as a shard does its batches: each wait ends
    std::vector<size_t> owner = shuffled(kBatches, 4);  // batch g belongs to thread owner[g] % kThreads
    std::vector<std::thread> ts;
    for (int t = 0; t < kThreads; t++)
        ts.emplace_back([&, t] {
            for (size_t g = 0; g < kBatches; g++)
                if ((int)(owner[g] % kThreads) == t && chain.chain(g, rows[g], &fake[g]) != TFBS_OK) bad++;
        });
    for (auto &t : ts) t.join();
    CHECK(bad == 0);
    uint64_t want = 1;
    for (size_t g = 0; g < kBatches; g++) {
        CHECK(fake[g] == want);
        want += rows[g];
    }
}

void chain_abort_wakes_a_waiter() {
    tfbs::PosChain chain(4);
    uint32_t fake = 0;
    // batch 2's predecessor never comes
    std::atomic<bool> entering(false);
    auto waiter = std::async(std::launch::async, [&] {
        entering = true;
        return chain.chain(2, 10, &fake);
    });
    while (!entering) std::this_thread::yield();
    for (int i = 0; i < 1000; i++) std::this_thread::yield();  // (let it reach the wait; the result is the same either way)
    std::thread other([&] { chain.abort(); });
    const bool woke = waiter.wait_for(std::chrono::seconds(5)) == std::future_status::ready;
    other.join();
    if (!woke) {
        fprintf(stderr, "PosChain::abort did not wake the waiter within 5 s\n");
        fflush(stderr);
        _Exit(1);  // (the waiter cannot be joined)
    }
    CHECK(waiter.get() == TFBS_E_STATE);
    CHECK(fake == 0);
    uint32_t f0 = 0;
    CHECK(chain.chain(0, 1, &f0) == TFBS_E_STATE);  // and nobody chains after it
}

void whole_regions(const std::vector<size_t> &recs, size_t limit) {
    const size_t n = recs.size();
    std::vector<std::pair<size_t, size_t>> slices;
    const int rc = tfbs::for_whole_regions(n, [&](size_t r) { return recs[r]; }, limit, [&](size_t q0, size_t q1) {
        slices.push_back({q0, q1});
        return TFBS_OK;
    });
    CHECK(rc == TFBS_OK);
    size_t at = 0;
    for (auto &s : slices) {
        CHECK(s.first == at);      // consecutive
        CHECK(s.second > s.first);  // one region at least
        CHECK(s.second <= n);
        const size_t sum = std::accumulate(recs.begin() + (long)s.first, recs.begin() + (long)s.second, (size_t)0);
        CHECK(s.second - s.first == 1 || sum <= limit);
        if (s.second < n) CHECK(sum + recs[s.second] > limit);  // maximal: the next region would not have fitted
        at = s.second;
    }
    CHECK(at == n);  // and they cover [0, n)
    CHECK(n != 0 || slices.empty());
}

void whole_regions_cases() {
    const size_t limit = 100;
    whole_regions({}, limit);
    whole_regions(std::vector<size_t>(17, 0), limit);  // all zero: one slice
    whole_regions({limit + 1}, limit);
    whole_regions({3, limit + 50, 4, 5}, limit);  // a region larger than the limit between others
    whole_regions({40, 30, 30, 7, 7}, limit);      // a run whose sum is the limit exactly
    whole_regions({40, 30, 31, 7, 7}, limit);      // the same run plus one
    whole_regions({40, 30, 30}, limit);
    whole_regions({0, 0, limit, 0, 1, 0}, limit);
    std::vector<size_t> slices;
    // fn's failure stops the walk
    const int rc = tfbs::for_whole_regions(5, [](size_t) { return (size_t)1; }, 1, [&](size_t q0, size_t) {
        slices.push_back(q0);
        return q0 == 2 ? TFBS_E_ARG : TFBS_OK;
    });
    CHECK(rc == TFBS_E_ARG && slices.size() == 3);
    size_t calls = 0;
    tfbs::for_whole_regions(17, [](size_t) { return (size_t)0; }, limit, [&](size_t q0, size_t q1) {
        CHECK(q0 == 0 && q1 == 17);
        calls++;
        return TFBS_OK;
    });
    CHECK(calls == 1);
}

}  // namespace

int main() {
    sequencer_in_order();
    sequencer_failing_sink();
    chain_prefix_sums();
    chain_abort_wakes_a_waiter();
    whole_regions_cases();
    if (failures) fprintf(stderr, "%d check(s) failed\n", failures);
    else printf("run_order: ok\n");
    return failures ? 1 : 0;
}
