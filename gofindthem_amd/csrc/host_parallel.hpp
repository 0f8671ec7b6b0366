// host_parallel.hpp -- the group finder's host threads: the walk and rule evaluation of ProcessJsons, the rows of a device JSON
// batch turned into results, the result document of the C ABI.  A pool per call, joined before it returns.
//
// GFT_HOST_THREADS=<n> (environment, n > 0) sets the number of workers; without it, the machine's hardware threads, 16 at the
// most (4 when they cannot be told).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>

#include "gft_guard.hpp"

namespace gft {

inline unsigned host_threads() {
    if (const char* e = getenv("GFT_HOST_THREADS")) { const int v = atoi(e); if (v > 0) return (unsigned)v; }
    const unsigned hc = std::thread::hardware_concurrency();
    return hc ? std::min(hc, 16u) : 4u;
}

template <class F>
void parallel_for(uint64_t n, F&& body) {            // body(index, worker), in chunks of 64 indices
    const unsigned nt = (unsigned)std::min<uint64_t>(host_threads(), (n + 63) / 64);
    if (nt <= 1) { for (uint64_t i = 0; i < n; i++) body(i, 0u); return; }
    std::atomic<uint64_t> next(0);
    std::vector<std::thread> pool;
    pool.reserve(nt);
    // an exception inside a worker would be std::terminate: the first one is carried to the calling thread and thrown
    // again there (the entry point's barrier turns it into a status), the other workers stop taking work
    std::exception_ptr first;
    std::mutex first_mu;
    {
        gft::JoinAll joined(pool);           // (also when a worker could not be started)
        for (unsigned t = 0; t < nt; t++)
            pool.emplace_back([&, t]() noexcept {
                try {
                    for (;;) {
                        const uint64_t b = next.fetch_add(64);
                        if (b >= n) return;
                        for (uint64_t i = b; i < std::min(n, b + 64); i++) body(i, t);
                    }
                } catch (...) {
                    next.store(n);
                    std::lock_guard<std::mutex> g(first_mu);
                    if (!first) first = std::current_exception();
                }
            });
    }
    if (first) std::rethrow_exception(first);
}

}  // namespace gft
