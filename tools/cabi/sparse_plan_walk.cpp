// sparse_plan_walk.cpp -- a stand-alone walk of the planner's sparse outer planes (dashing_amd/csrc/plan.cpp, Tuning::
// sparse_planes) for a sanitizer build: random keys and per-sketch counts, every option value, row ranges, parts and small
// C(v) budgets, each plan held to its contract by dshh_plan_check_sparse (csrc/host/plan_capi.cpp).  Host code only.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/cabi/sparse_plan_walk \
//       tools/cabi/sparse_plan_walk.cpp dashing_amd/csrc/plan.cpp dashing_amd/csrc/host/plan_capi.cpp && tools/cabi/sparse_plan_walk
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

extern "C" int dshh_plan_check_sparse(uint64_t n, const uint32_t *keys, const uint32_t *gcnt, int mode, int want_sorted, uint64_t rb, uint64_t re,
                                      uint32_t nparts, int want_parts, int p, uint64_t cum_budget, uint32_t round_items, int sparse_planes,
                                      uint32_t sparse_cap, uint64_t *stats, uint32_t *routes, uint64_t routes_cap, char *err, size_t cap);

int main()
{
    std::mt19937_64 rng(12345);
    uint64_t plans = 0, routed = 0;
    for (int trial = 0; trial < 60; ++trial) {
        const int p = 9 + (int)(rng() % 8);  // 9 .. 16
        const uint64_t n = 1 + rng() % 900;
        const int q1 = 64 - p + 1;
        std::vector<uint32_t> keys(n), g(n);
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t lo = (uint32_t)(rng() % 6), L = lo + (uint32_t)(rng() % 3), T = L + (uint32_t)(rng() % 4);
            const uint32_t hi = std::min<uint32_t>((uint32_t)q1, T + (uint32_t)(rng() % 5));
            keys[i] = hi << 18 | std::min(T, hi) << 12 | std::min(L, hi) << 6 | std::min(lo, hi);
            // (mostly sets that fit a cap; now and then a saturated count, which keeps its block dense)
            const uint32_t g0 = (uint32_t)(trial % 4 == 3 && rng() % 50 == 0 ? rng() % 70000 : rng() % 900), g1 = g0 + (uint32_t)(rng() % 300);
            g[i] = std::min<uint32_t>(g0, 65535) | std::min<uint32_t>(g1, 65535) << 16;
        }
        const uint64_t nt = (n + 127) / 128;
        std::vector<uint32_t> routes(5 * nt * (nt + 1) / 2 + 5);
        for (int sp = -1; sp <= 2; ++sp) {
            const uint64_t rb = trial % 3 == 0 ? rng() % n : 0, re = trial % 3 == 0 ? rb + rng() % (n - rb + 1) : n;
            const int want_parts = trial % 4 == 1;
            const uint64_t budget = trial % 5 == 2 ? (uint64_t)(1 + rng() % 8) << 20 : (uint64_t)8 << 30;
            const uint32_t cap = (uint32_t)(trial % 2 ? 900 + rng() % 1200 : rng() % 2100);
            uint64_t stats[12] = {0};
            char err[512] = {0};
            if (dshh_plan_check_sparse(n, keys.data(), trial % 7 == 6 ? nullptr : g.data(), 0, 1, rb, re, want_parts ? 1 + (uint32_t)(rng() % 5) : 1,
                                       want_parts, p, budget, rng() % 2 ? 768 : 512, sp, cap, stats, routes.data(), routes.size() / 5, err, sizeof err)) {
                std::fprintf(stderr, "trial %d (n %llu, p %d, sparse_planes %d, cap %u): %s\n", trial, (unsigned long long)n, p, sp, cap, err);
                return 1;
            }
            ++plans;
            routed += stats[10];
        }
    }
    std::printf("%llu plans checked, %llu planes routed sparse\n", (unsigned long long)plans, (unsigned long long)routed);
    return 0;
}
