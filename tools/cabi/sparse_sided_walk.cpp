// sparse_sided_walk.cpp -- a stand-alone walk of the planner's sided route (dashing_amd/csrc/plan.cpp, Tuning::sparse_sided)
// for a sanitizer build: random keys, per-sketch counts and thresholds, every setting of the two options, row ranges, parts,
// small C(v) budgets and stale caps, each plan held to its contract by dshh_plan_check_sparse_sided
// (csrc/host/plan_capi.cpp).  Host code only.
//
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o tools/cabi/sparse_sided_walk \
//       tools/cabi/sparse_sided_walk.cpp dashing_amd/csrc/plan.cpp dashing_amd/csrc/host/plan_capi.cpp && tools/cabi/sparse_sided_walk
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

extern "C" int dshh_plan_check_sparse_sided(uint64_t n, const uint32_t *keys, const uint32_t *gcnt, const uint32_t *thr, uint32_t thr_cap, int mode,
                                            int want_sorted, uint64_t rb, uint64_t re, uint32_t nparts, int want_parts, int p, uint64_t cum_budget,
                                            uint32_t round_items, int sparse_planes, int sparse_sided, uint32_t sparse_cap, uint64_t *stats,
                                            uint32_t *routes, uint64_t routes_cap, uint32_t *items, uint64_t items_cap, uint32_t *slabs,
                                            uint64_t slabs_cap, char *err, size_t cap);

int main()
{
    std::mt19937_64 rng(54321);
    uint64_t plans = 0, routed = 0, sided = 0, transposed = 0, tables = 0;
    for (int trial = 0; trial < 80; ++trial) {
        const int p = 11 + (int)(rng() % 6);  // 11 .. 16
        const uint64_t n = 1 + rng() % 900;
        const int q1 = 64 - p + 1;
        const uint32_t cap = (uint32_t)(trial % 2 ? 900 + rng() % 1100 : rng() % 2041);
        std::vector<uint32_t> keys(n), g(n), thr(n);
        for (uint64_t i = 0; i < n; ++i) {
            const uint32_t lo = (uint32_t)(rng() % 6), L = lo + (uint32_t)(rng() % 3), T = L + (uint32_t)(rng() % 5);
            const uint32_t hi = std::min<uint32_t>((uint32_t)q1, T + (uint32_t)(rng() % 5));
            const uint32_t Tk = std::min(T, hi), Lk = std::min(L, hi);
            keys[i] = hi << 18 | Tk << 12 | Lk << 6 | std::min(lo, hi);
            const uint32_t g0 = (uint32_t)(rng() % 1500), g1 = g0 + (uint32_t)(rng() % 900);
            g[i] = g0 | g1 << 16;
            // thresholds that agree with the counts at this cap: vU at or below the lowest plane the counts let through
            const uint32_t vU = g1 <= cap ? (Tk ? Tk - 1 : 0) - std::min<uint32_t>(Tk ? Tk - 1 : 0, (uint32_t)(rng() % 3))
                                : g0 <= cap ? Tk : Tk + 1 + (uint32_t)(rng() % 3);
            const uint32_t vA = std::min<uint32_t>(vU ? vU - 1 : 0, Lk + (uint32_t)(rng() % 4));
            thr[i] = vU | vA << 8;
        }
        const uint64_t nt = (n + 127) / 128, ntiles = nt * (nt + 1) / 2;
        std::vector<uint32_t> routes(6 * ntiles + 6), items(5 * 64 * ntiles + 5), slabs(3 * 64 * nt + 3);
        for (int sd = -1; sd <= 1; ++sd)
            for (int sp = -1; sp <= 2; ++sp) {
                const uint64_t rb = trial % 3 == 0 ? rng() % n : 0, re = trial % 3 == 0 ? rb + rng() % (n - rb + 1) : n;
                const int want_parts = trial % 4 == 1;
                const uint64_t budget = trial % 5 == 2 ? (uint64_t)(1 + rng() % 8) << 20 : (uint64_t)8 << 30;
                const uint32_t plan_cap = trial % 9 == 8 ? cap / 2 : cap;  // (a stale cap: the sided route stays off)
                uint64_t stats[15] = {0};
                char err[512] = {0};
                if (dshh_plan_check_sparse_sided(n, keys.data(), g.data(), trial % 7 == 6 ? nullptr : thr.data(), cap, 0, 1, rb, re,
                                                 want_parts ? 1 + (uint32_t)(rng() % 5) : 1, want_parts, p, budget, rng() % 2 ? 768 : 512, sp, sd, plan_cap,
                                                 stats, routes.data(), ntiles + 1, items.data(), 64 * ntiles + 1, slabs.data(), 64 * nt + 1, err, sizeof err)) {
                    std::fprintf(stderr, "trial %d (n %llu, p %d, sparse_planes %d, sparse_sided %d, cap %u): %s\n", trial, (unsigned long long)n, p, sp, sd,
                                 plan_cap, err);
                    return 1;
                }
                if ((plan_cap != cap || p < 13) && stats[12]) {
                    std::fprintf(stderr, "trial %d: the sided route planned on a stale cap or below p = 13\n", trial);
                    return 1;
                }
                ++plans;
                routed += stats[10], sided += stats[12], transposed += stats[13], tables += stats[14];
            }
    }
    std::printf("%llu plans checked, %llu planes routed sparse (%llu by the sided route, %llu transposed), %llu table-only slabs\n",
                (unsigned long long)plans, (unsigned long long)routed, (unsigned long long)sided, (unsigned long long)transposed,
                (unsigned long long)tables);
    return 0;
}
