// unionfind_check.cpp -- csrc/oa_unionfind.hpp on the host: 16 threads link random edge lists into one parent array without ever
// waiting for each other; afterwards every vertex's root must be the LOWEST index of its component, as a sequential union-find
// over the same edges finds it.  Built by tests/test_clustering.py with -fsanitize=thread where the toolchain has it.
// Exit status 0 and a last line "OK" when every round agrees.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <utility>
#include <vector>

#include "oa_unionfind.hpp"

namespace {

struct HostAtomics {
    static uint32_t load(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
    static uint32_t cas(uint32_t *p, uint32_t want, uint32_t v)
    {
        __atomic_compare_exchange_n(p, &want, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
        return want;                                                 // (what was there: `want` itself on success)
    }
    static void fetch_min(uint32_t *p, uint32_t v)
    {
        uint32_t cur = __atomic_load_n(p, __ATOMIC_RELAXED);
        while (v < cur && !__atomic_compare_exchange_n(p, &cur, v, true, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    }
};

uint32_t seq_find(std::vector<uint32_t> &p, uint32_t x)
{
    while (p[x] != x) { p[x] = p[p[x]]; x = p[x]; }
    return x;
}

constexpr int THREADS = 16;

// n vertices, m random edges (chain = true: also the path 0 - 1 - ... - n - 1 in a shuffled order, the deepest trees there are)
bool round_ok(uint32_t n, size_t m, bool chain, unsigned seed)
{
    std::mt19937 rng(seed);
    std::vector<std::pair<uint32_t, uint32_t>> edges;
    for (size_t e = 0; e < m; ++e) edges.emplace_back((uint32_t)(rng() % n), (uint32_t)(rng() % n));
    if (chain) for (uint32_t i = 0; i + 1 < n; ++i) if (i % 500 != 499) edges.emplace_back(i, i + 1);
    std::shuffle(edges.begin(), edges.end(), rng);

    std::vector<uint32_t> parent(n), ref(n);
    for (uint32_t i = 0; i < n; ++i) parent[i] = ref[i] = i;
    const int max_steps = (int)(2 * n + 64);
    int spent[THREADS] = { 0 };
    std::vector<std::thread> pool;
    for (int t = 0; t < THREADS; ++t)
        pool.emplace_back([&, t] {
            for (size_t e = (size_t)t; e < edges.size(); e += THREADS) {
                int budget = max_steps;
                const uint32_t a = oa::uf_find_compress<HostAtomics>(parent.data(), edges[e].first, budget);
                oa::uf_link<HostAtomics>(parent.data(), a, edges[e].second, budget);
                if (budget <= 0) spent[t] = 1;
            }
        });
    for (auto &th : pool) th.join();

    for (const auto &e : edges) {
        const uint32_t a = seq_find(ref, e.first), b = seq_find(ref, e.second);
        if (a != b) ref[std::max(a, b)] = std::min(a, b);             // (the lower root stays: the root is the lowest index)
    }
    for (int t = 0; t < THREADS; ++t) if (spent[t]) { std::printf("a budget of %d steps ran out (thread %d)\n", max_steps, t); return false; }
    for (uint32_t i = 0; i < n; ++i) {
        if (parent[i] > i) { std::printf("parent[%u] = %u rose\n", i, parent[i]); return false; }
        int budget = max_steps;
        const uint32_t got = oa::uf_find<HostAtomics>(parent.data(), i, budget), want = seq_find(ref, i);
        if (got != want) { std::printf("n %u m %zu seed %u: root of %u is %u, sequential %u\n", n, m, seed, i, got, want); return false; }
    }
    return true;
}

}  // namespace

int main()
{
    unsigned seed = 1;
    for (uint32_t n : { 2u, 17u, 300u, 3000u, 20000u })
        for (size_t per : { 1u, 2u, 8u })
            for (int chain = 0; chain < 2; ++chain, ++seed)
                if (!round_ok(n, (size_t)n * per / 2, chain != 0, seed)) return 1;
    std::printf("OK\n");
    return 0;
}
