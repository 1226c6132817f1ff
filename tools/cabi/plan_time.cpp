// plan_time.cpp -- the host planner of the compare path (dashing_amd/csrc/plan.cpp) timed phase by phase, CPU only, one
// thread: build_layout, build_tiles with the sparse routes off and automatic, emit_sparse_items, build_band_items over all
// bands and emit_tile_lists, on synthetic keys, counts and thresholds (the generator of sparse_sided_walk.cpp, thresholds
// that agree with the counts at the default cap; round 768 / small round 512 as engine.hip plans under pair_groups = auto).
// The inputs are NOT the bench's sketches: they route more planes than real data of the same shape, so compare per item.
// One line per shape: the median of `reps` repetitions of every phase in microseconds, and what was planned.
//
//   g++ -O2 -std=c++17 -I dashing_amd/csrc -o tools/cabi/plan_time tools/cabi/plan_time.cpp dashing_amd/csrc/plan.cpp && tools/cabi/plan_time
//   (sanitizers, at a small size: -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all, then  tools/cabi/plan_time 21 700 14)
// Arguments: [reps (at least 21, default 31)] [n p] -- one shape instead of the four recorded ones.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "plan.h"

using namespace dsh;
using namespace dsh::plan;

namespace {

double median(std::vector<double> v)
{
    std::sort(v.begin(), v.end());
    return v[v.size() / 2];
}

template <class F>
double time_us(F &&f)
{
    const auto t0 = std::chrono::steady_clock::now();
    f();
    return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

void one_shape(uint64_t n, int p, int reps)
{
    std::mt19937_64 rng(54321 + n + (uint64_t)p);
    const int q1 = 64 - p + 1;
    const uint32_t cap = kSparseCapDefault;
    std::vector<uint32_t> keys(n), g(n), thr(n);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t lo = (uint32_t)(rng() % 6), L = lo + (uint32_t)(rng() % 3), T = L + (uint32_t)(rng() % 5);
        const uint32_t hi = std::min<uint32_t>((uint32_t)q1, T + (uint32_t)(rng() % 5));
        const uint32_t Tk = std::min(T, hi), Lk = std::min(L, hi);
        keys[i] = hi << 18 | Tk << 12 | Lk << 6 | std::min(lo, hi);
        const uint32_t g0 = (uint32_t)(rng() % 1500), g1 = g0 + (uint32_t)(rng() % 900);
        g[i] = g0 | g1 << 16;
        const uint32_t vU = g1 <= cap ? (Tk ? Tk - 1 : 0) - std::min<uint32_t>(Tk ? Tk - 1 : 0, (uint32_t)(rng() % 3)) : g0 <= cap ? Tk : Tk + 1 + (uint32_t)(rng() % 3);
        const uint32_t vA = std::min<uint32_t>(vU ? vU - 1 : 0, Lk + (uint32_t)(rng() % 4));
        thr[i] = vU | vA << 8;
    }
    std::vector<uint64_t> parts;
    range_parts(n, 0, n, 1, parts);
    const SketchWords words{keys.data(), g.data(), thr.data(), cap};
    const LayoutQuery query{1, 0, n, &parts, 0, nullptr};
    Tuning tu;
    tu.W = (uint32_t)std::max<uint64_t>(1, (1ull << p) / 32);
    tu.kc = tu.W >= 32 ? 32 : 16;
    tu.cum_bytes = p <= 15 ? 2 : 4;
    tu.lockstep = tu.W >= (uint32_t)tu.kc;
    tu.round_items = 768;
    tu.small_round_items = 512;
    tu.p = p;
    tu.sparse_cap = cap;
    PairQuery q;
    q.row_end = n;
    Layout L;
    PairPlan pp;  // (kept over the repetitions, as a context keeps it over its calls: the scratch is warm)
    std::vector<double> t_layout, t_off, t_auto, t_emit, t_items, t_lists;
    std::vector<U4> dt, df;
    for (int r = 0; r < reps; ++r) {
        t_layout.push_back(time_us([&] { build_layout(n, words, query, L); }));
        tu.sparse_planes = 0, tu.sparse_sided = 0;
        t_off.push_back(time_us([&] { build_tiles(L, q, tu, pp); }));
        tu.sparse_planes = -1, tu.sparse_sided = -1;
        t_auto.push_back(time_us([&] { build_tiles(L, q, tu, pp); }));
        t_emit.push_back(time_us([&] { emit_sparse_items(L, pp); }));
        t_items.push_back(time_us([&] {
            for (size_t bi = 0; bi < pp.bands.size(); ++bi) build_band_items(tu, pp, bi);
        }));
        dt.resize(pp.T.size()), df.resize(pp.T.size());
        t_lists.push_back(time_us([&] { emit_tile_lists(L, pp, dt.data(), df.data()); }));
    }
    const double emit = median(t_emit);
    std::printf("{\"n\": %llu, \"p\": %d, \"reps\": %d, \"tiles\": %zu, \"bands\": %zu, \"dense_items\": %zu, \"sparse_items\": %zu, \"slabs\": %zu, "
                "\"build_layout_us\": %.1f, \"build_tiles_routes_off_us\": %.1f, \"build_tiles_routes_auto_us\": %.1f, \"emit_sparse_items_us\": %.1f, "
                "\"emit_ns_per_item\": %.2f, \"build_band_items_us\": %.1f, \"emit_tile_lists_us\": %.1f}\n",
                (unsigned long long)n, p, reps, pp.T.size(), pp.bands.size(), pp.items.size(), pp.sp_items.size(), pp.slabs.size(), median(t_layout),
                median(t_off), median(t_auto), emit, pp.sp_items.empty() ? 0.0 : 1000.0 * emit / (double)pp.sp_items.size(), median(t_items),
                median(t_lists));
}

}  // namespace

int main(int argc, char **argv)
{
    const int reps = std::max(21, argc > 1 ? std::atoi(argv[1]) : 31);
    if (argc > 3) {
        one_shape((uint64_t)std::atoll(argv[2]), std::atoi(argv[3]), reps);
        return 0;
    }
    one_shape(10000, 14, reps);
    one_shape(5000, 16, reps);
    one_shape(30000, 14, reps);
    one_shape(100000, 10, reps);
    return 0;
}
