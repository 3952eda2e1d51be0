// InBlocks.h — a loop over [0, n) in blocks that threads take in turn: the host's share of the super-read calls (hc_api_sr.cpp) and
// their host mirrors (SrConsensus.cpp, SrSelfOverlap.cpp).
#pragma once
#include <algorithm>
#include <atomic>
#include <cstdint>
#include <thread>
#include <vector>

namespace hc {

// `work(a, b)` for every block [a, b) of [0, n), on up to n_threads threads (at most 64, at most one per block; the caller is one of them)
template <typename F>
void in_blocks(uint64_t n, uint64_t block, unsigned n_threads, F work) {
    const uint64_t n_blocks = (n + block - 1) / block;
    const unsigned T = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>({(uint64_t)n_threads, 64, n_blocks}));
    std::atomic<uint64_t> turn{0};
    auto run = [&]() {
        for (uint64_t b = turn.fetch_add(1); b < n_blocks; b = turn.fetch_add(1)) work(b * block, std::min(n, (b + 1) * block));
    };
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; t++) th.emplace_back(run);
    run();
    for (auto& x : th) x.join();
}

}  // namespace hc
