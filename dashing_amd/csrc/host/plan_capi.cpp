// plan_capi.cpp -- CPU test hook of the pure-host planner (../plan.cpp): builds a layout and a pair plan for given
// per-sketch keys exactly as engine.hip does and checks the plan against its contract, so the schedule that replaces
// dist_loop / perform_core_op (src/sketch_and_cmp.h:785-880, :699-710) is unit-tested without a GPU
// (tests/test_plan.py).  Also the sequential build of the clusters' union-find (dsh_plan_uf_labels, at the end) and the band rule of
// the greedy representatives (dshh_greedy_bands) and the band walk all five band consumers share (dshh_threshold_bands), and the
// sequential build of the linkage clusters (dsh_plan_linkage_labels, dsh_plan_linkage_loose: ../linkage.h), and the sketch
// path's planners (dshh_sketch_plan: ../sketch_plan.h), and the union curve's (dshh_curve_plan: ../curve_plan.h), and the exchange's round schedule
// (dshh_exchange_plan: ../exchange_plan.h).  Built into libdashing_host.so; not part of the GPU C-ABI.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../linkage.h"
#include "../mst.h"
#include "../plan.h"
#include "../sketch_plan.h"
#include "../uf.h"

using namespace dsh;
using namespace dsh::plan;

namespace {

// sparse outer planes (plan.h, Tuning): what dshh_plan_check_sparse adds to a check -- the per-sketch counts, the two
// options, and where the routes go (5 words per tile: row block, column block, plane begin, plane end, planes routed sparse)
struct SparseCheck {
    const uint32_t *gcnt = nullptr;
    int planes = 0;
    uint32_t cap = 0;
    uint32_t *routes = nullptr;
    uint64_t routes_cap = 0;  // tiles `routes` has room for
    // the sided route (dshh_plan_check_sparse_sided): the per-sketch thresholds vU | vA << 8 and their cap, the option, and
    // where the routes, items and slabs go -- 6 words per tile (row block, column block, plane begin, plane end, planes
    // routed below, planes routed above), 5 per item (tile, plane, list A | table A << 1 | transposed << 2, slab of the row
    // block, slab of the column block), 3 per slab (block, plane, A | table-only << 1)
    const uint32_t *thr = nullptr;
    uint32_t thr_cap = 0;
    int sided = 0;
    uint32_t *routes6 = nullptr, *items5 = nullptr, *slabs3 = nullptr;
    uint64_t items_cap = 0, slabs_cap = 0;
    uint32_t max_slabs = 0;  // Tuning::sparse_max_slabs (dshh_plan_sparse_items); 0 = the planner's default
};

struct Err {
    char *buf;
    size_t cap;
    int fail(const char *fmt, ...)
    {
        if (buf && cap) {
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(buf, cap, fmt, ap);
            va_end(ap);
        }
        return -1;
    }
};

// What an entry point asks plan_check for.
// mode: 0 triangle rows [rb, re) (want_sorted decides the layout), 1 rectangle rows [rb,re) x cols [cb,ce) (identity
// layout), 2 sorted_rows (whole sorted layout, rows [rb,re) index plane columns: shards / band-wise kNN), 3 triangle
// rows in ROW-SORTED parts (the wanted rows one key-ordered run, parts = runs of whole tile rows of that order).
// stats out: [0] tiles, [1] bands, [2] items, [3] parts with an event, [4] planes per tile x 100, [5] Npad, [6] P,
// [7] rounds summed over the bands, each in its own round (a round of fragments counted as one), [8] overflow fragments,
// [9] the round the first band was planned for, [10] sparse items, [11] slabs, [12] items of the sided route,
// [13] transposed items, [14] table-only slabs -- as many of them as the entry point's caller has slots for (stats_slots).
struct CheckJob {
    uint64_t n = 0;
    const uint32_t *keys = nullptr;
    int mode = 0, want_sorted = 0;
    uint64_t rb = 0, re = 0, cb = 0, ce = 0;
    uint32_t nparts = 1;
    int want_parts = 0, p = 0;
    uint64_t cum_budget = 0;
    int lockstep = 1, nsplit = 0, ls_item_chunks = 64;
    std::vector<uint64_t> extra;  // further wanted segments {b0, e0, ...} (plan.h, row sets; modes 0 and 3 with a sorted layout only)
    uint32_t round_items = 0;     // the tile kernel's round (256 x the items per workgroup, engine.hip); 0 = the planner's default
    const SparseCheck *sc = nullptr;
    uint64_t *stats = nullptr;
    int stats_slots = 9;
    // (resolve()) the layout's wanted range, and mode 3 spelled out
    bool rowsorted = false;
    uint64_t lrb = 0, lre = 0;

    void resolve()
    {
        if (re > n) re = n;
        rowsorted = mode == 3;
        if (rowsorted) mode = 0, want_sorted = 1, want_parts = 1;
        if (mode == 1 || !want_sorted) want_sorted = mode == 2 ? 1 : 0;
        if (mode == 2) want_sorted = 1;
        lrb = 0, lre = n;
        if (want_sorted && mode == 0) lrb = rb, lre = re;
    }
    bool plan_parts() const { return want_parts && mode == 0 && want_sorted; }
    // the wanted segments in the wanted order: extra segments first, then the main range
    std::vector<std::pair<uint64_t, uint64_t>> wanted_segments() const
    {
        std::vector<std::pair<uint64_t, uint64_t>> wsegs;
        wanted_order(n, lrb, lre, &extra, wsegs, rowsorted);
        return wsegs;
    }
};

bool in_rows(const std::vector<std::pair<uint64_t, uint64_t>> &wsegs, uint64_t i)
{
    for (auto &w : wsegs)
        if (i >= w.first && i < w.second) return true;
    return false;
}

uint32_t chunks_per_plane(const Tuning &tu) { return tu.W >= (uint32_t)tu.kc ? tu.W / tu.kc : 1; }

// layout, options and plan of a resolved job, exactly as engine.hip makes them
void job_layout(const CheckJob &job, Layout &L)
{
    std::vector<uint64_t> parts;
    if (job.want_sorted && !job.rowsorted) range_parts(job.n, job.lrb, job.lre, std::max<uint32_t>(job.want_parts ? job.nparts : 1, 1), parts);
    const SparseCheck *sc = job.sc;
    const SketchWords words{job.keys, sc ? sc->gcnt : nullptr, sc ? sc->thr : nullptr, sc ? sc->thr_cap : 0};
    const LayoutQuery query{job.want_sorted, job.lrb, job.lre, &parts, job.rowsorted ? std::max<uint32_t>(job.nparts, 1) : 0,
                            job.extra.empty() ? nullptr : &job.extra};
    build_layout(job.n, words, query, L);
}

// two_step: build_tiles, emit_sparse_items and the bands' items one after the other, as engine.hip calls them
bool job_plan(const CheckJob &job, const Layout &L, Tuning &tu, PairQuery &q, PairPlan &pp, bool two_step = false)
{
    const uint64_t m = 1ull << job.p;
    tu.W = (uint32_t)std::max<uint64_t>(1, m / 32);
    tu.kc = tu.W >= 32 ? 32 : 16;
    tu.cum_bytes = job.p <= 15 ? 2 : 4;
    tu.cum_budget = job.cum_budget;
    tu.nsplit = job.nsplit;
    tu.lockstep = job.lockstep && tu.W >= (uint32_t)tu.kc;
    tu.ls_item_chunks = job.ls_item_chunks;
    if (job.round_items) tu.round_items = job.round_items;
    if (job.round_items > 512) tu.small_round_items = 512;  // (as engine.hip under pair_groups = auto)
    tu.p = job.p;
    if (job.sc) tu.sparse_planes = job.sc->planes, tu.sparse_cap = job.sc->cap, tu.sparse_sided = job.sc->sided;
    if (job.sc && job.sc->max_slabs) tu.sparse_max_slabs = job.sc->max_slabs;
    q.rect = job.mode == 1;
    q.sorted_rows = job.mode == 2;
    q.want_parts = job.plan_parts();
    q.row_begin = job.rb;
    q.row_end = job.re;
    q.col_begin = job.cb;
    q.col_end = job.ce;
    if (!two_step) return build_pairs(L, q, tu, pp);
    if (!build_tiles(L, q, tu, pp)) return false;
    for (size_t bi = 0; bi < pp.bands.size(); ++bi) {  // (the dense path first: it must not need the emission)
        if (bi == 1) emit_sparse_items(L, pp);
        build_band_items(tu, pp, bi);
    }
    if (pp.bands.size() < 2) emit_sparse_items(L, pp);
    return true;
}

// ---- the checks: each returns at its first failure ---------------------------------------------------------------------

// row-sorted: one key-ordered run per wanted segment, cuts on whole tile rows of the wanted order, row offsets of the rank's buffer
int check_rowsorted(const CheckJob &job, const Layout &L, Err &E)
{
    const uint64_t n = job.n, lrb = job.lrb;
    const uint32_t *keys = job.keys;
    const auto wsegs = job.wanted_segments();
    uint64_t nw = 0, wspan = 0;
    for (auto &w : wsegs) nw += w.second - w.first, wspan += tri_span(n, w.first, w.second);
    auto skey = [&](uint32_t g) { return ((uint32_t)key_T(keys[g]) << 12) | ((uint32_t)key_L(keys[g]) << 6) | (uint32_t)key_hi(keys[g]); };
    for (auto &w : wsegs)
        for (uint64_t s = w.first - lrb + 1; s < w.second - lrb; ++s)
            if (skey(L.perm[s - 1]) > skey(L.perm[s])) return E.fail("row-sorted: a wanted segment is not one key-ordered run at %llu", (unsigned long long)s);
    if (L.part_w.empty() || L.part_w.front() != 0 || L.part_w.back() != nw) return E.fail("row-sorted: part cuts do not span the wanted rows");
    for (size_t q = 1; q + 1 < L.part_w.size(); ++q) {  // every cut at the start of a tile row of the wanted order
        if (L.part_w[q] <= L.part_w[q - 1]) return E.fail("row-sorted: cut %zu at %llu", q, (unsigned long long)L.part_w[q]);
        uint64_t w0 = 0;
        bool ok = false;
        for (auto &w : wsegs) {
            if (L.part_w[q] >= w0 && L.part_w[q] < w0 + (w.second - w.first)) ok = (L.part_w[q] - w0) % kTile == 0;
            w0 += w.second - w.first;
        }
        if (!ok) return E.fail("row-sorted: cut %zu at %llu is not at a tile row of the wanted order", q, (unsigned long long)L.part_w[q]);
    }
    if (L.part_w.size() - 1 > std::max<uint32_t>(job.nparts, 1)) return E.fail("row-sorted: more parts than asked for");
    uint64_t acc = 0, w_ = 0;
    if (L.rowoff_w.size() != nw + 1) return E.fail("row-sorted: rowoff_w size");
    for (auto &w : wsegs)
        for (uint64_t s = w.first - lrb; s < w.second - lrb; ++s, ++w_) {
            if (s >= L.rowoff.size() || L.rowoff[s] != acc || L.rowoff_w[w_] != acc) return E.fail("row-sorted: rowoff[%llu]", (unsigned long long)s);
            acc += n - 1 - L.perm[s];
        }
    if (L.rowoff_w.back() != acc || acc != wspan) return E.fail("row-sorted: the rows do not add up to the span");
    return 0;
}

// layout: perm is a permutation of the columns; the parts hold exactly their rows; block stats are right
int check_layout(const CheckJob &job, const Layout &L, Err &E)
{
    const uint64_t n = job.n, lrb = job.lrb, lre = job.lre;
    const auto wsegs = job.wanted_segments();
    const uint64_t col0 = job.want_sorted ? lrb : 0;
    if (L.ncols != n - col0) return E.fail("ncols %llu != %llu", (unsigned long long)L.ncols, (unsigned long long)(n - col0));
    if (L.Npad % kTile || L.Npad < L.ncols || L.Npad >= L.ncols + kTile) return E.fail("bad Npad %u", L.Npad);
    std::vector<uint8_t> seen(n, 0);
    for (uint64_t s = 0; s < L.ncols; ++s) {
        const uint32_t g = L.perm[s];
        if (g < col0 || g >= n || seen[g]) return E.fail("perm[%llu] = %u is out of range or repeated", (unsigned long long)s, g);
        seen[g] = 1;
    }
    if (!job.want_sorted) return 0;
    uint64_t s = 0;
    for (size_t q = 0; q + 1 < L.parts.size(); ++q)
        for (uint64_t r = L.parts[q]; r < L.parts[q + 1]; ++r, ++s)
            if (L.perm[s] < L.parts[q] || L.perm[s] >= L.parts[q + 1])
                return E.fail("column %llu holds sketch %u, not a row of part %zu", (unsigned long long)s, L.perm[s], q);
    if (!job.rowsorted && job.extra.empty()) {
        if (L.part_pos.size() != L.parts.size()) return E.fail("part positions and parts differ in number");
        for (size_t q = 0; q < L.parts.size(); ++q)
            if (L.part_pos[q] != L.parts[q] - lrb) return E.fail("part position %zu", q);
    }
    for (; s < L.ncols; ++s)
        if (L.perm[s] < lre) return E.fail("column %llu (after the wanted rows) holds wanted row %u", (unsigned long long)s, L.perm[s]);
    // every run holds exactly its rows: a wanted segment's positions hold its rows; every block is wanted or not as a whole
    for (auto &w : wsegs)
        for (uint64_t s2 = w.first - lrb; s2 < w.second - lrb; ++s2)
            if (L.perm[s2] < w.first || L.perm[s2] >= w.second) return E.fail("position %llu of a wanted segment holds row %u", (unsigned long long)s2, L.perm[s2]);
    if (!job.extra.empty())
        for (uint64_t s2 = 0; s2 < L.ncols; ++s2) {
            // rows to the right of a position are larger unless they share its run: position order = row order between runs
            const uint64_t b = s2 / kTile * kTile;
            if (in_rows(wsegs, L.perm[s2]) != in_rows(wsegs, L.perm[b])) return E.fail("block %llu mixes wanted and other rows", (unsigned long long)(b / kTile));
        }
    if (L.whole)
        for (uint64_t i = 0; i < n; ++i)
            if (L.perm[n + L.perm[i]] != i) return E.fail("inverse permutation wrong at %llu", (unsigned long long)i);
    return 0;
}

// the pairs the job wants
uint64_t wanted_pairs(const CheckJob &job)
{
    const uint64_t n = job.n, rb = job.rb, re = job.re;
    if (job.mode == 1) return (re > rb ? re - rb : 0) * (job.ce > job.cb ? job.ce - job.cb : 0);
    uint64_t wanted = 0;
    for (uint64_t i = rb; i < re; ++i) wanted += n - 1 - i;
    if (job.mode == 2) return wanted;  // (rows of the layout: si = rb .. re - 1)
    for (size_t x = 0; x + 1 < job.extra.size(); x += 2)
        for (uint64_t i = job.extra[x]; i < job.extra[x + 1]; ++i) wanted += n - 1 - i;
    return wanted;
}

// coverage: every wanted pair is owned by exactly one (tile, lane) -- the `active` predicate of k_finalize
int check_coverage(const CheckJob &job, const Layout &L, const PairPlan &pp, Err &E)
{
    const uint64_t n = job.n, rb = job.rb, re = job.re, cb = job.cb, ce = job.ce;
    const int mode = job.mode;
    const uint32_t *keys = job.keys;
    const std::vector<uint64_t> &extra = job.extra;
    const auto wsegs = job.wanted_segments();
    const uint64_t wanted = wanted_pairs(job);
    std::vector<uint8_t> hit(mode == 1 ? wanted : n * n, 0);
    uint64_t got = 0;
    for (const U4 &t : pp.T) {
        if (t.z > t.w || t.w > L.P) return E.fail("tile (%u,%u) has the plane range [%u,%u) of %u", t.x, t.y, t.z, t.w, L.P);
        for (uint32_t a = 0; a < kTile; ++a)
            for (uint32_t b = 0; b < kTile; ++b) {
                const uint64_t si = (uint64_t)t.x * kTile + a, sj = (uint64_t)t.y * kTile + b;
                if (si >= L.ncols || sj >= L.ncols) continue;
                const uint64_t i = L.perm[si], j = L.perm[sj];
                bool active;
                uint64_t slot;
                if (mode == 1) {
                    active = i >= rb && i < re && j >= cb && j < ce;
                    slot = active ? (i - rb) * (ce - cb) + (j - cb) : 0;
                } else if (mode == 2) {
                    active = si < sj && si >= rb && si < re;
                    slot = si * n + sj;
                } else {
                    // (k_finalize: with extra segments run_pairs hands it the rows [rb, n) -- every pair of a launched tile)
                    const uint64_t oi = std::min(i, j), oj = std::max(i, j);
                    active = si < sj && oi >= rb && oi < (extra.empty() ? re : n);
                    slot = oi * n + oj;
                    if (active && !extra.empty() && !in_rows(wsegs, oi))
                        return E.fail("tile (%u,%u) computes the pair (%llu,%llu) of a row this rank does not hold", t.x, t.y, (unsigned long long)oi, (unsigned long long)oj);
                }
                if (!active) continue;
                if (hit[slot]++) return E.fail("pair slot %llu computed twice (tile %u,%u)", (unsigned long long)slot, t.x, t.y);
                ++got;
                // exactness of the tile's dense range for this pair: everything above T is listed by
                // one of the two sketches, everything below Lp is below both low thresholds or below both minima
                const uint32_t ka = keys[i], kb = keys[j];
                const int Tp = L.pbase + (int)t.w, Lp = L.pbase + (int)t.z;
                if (Tp < std::max(key_T(ka), key_T(kb))) return E.fail("tile (%u,%u): T %d below a sketch's threshold", t.x, t.y, Tp);
                if (Lp > std::max(std::max(key_lo(ka), key_lo(kb)), std::min(key_L(ka), key_L(kb))))
                    return E.fail("tile (%u,%u): Lp %d above what the low lists cover", t.x, t.y, Lp);
            }
    }
    if (got != wanted) return E.fail("%llu of %llu wanted pairs are covered", (unsigned long long)got, (unsigned long long)wanted);
    return 0;
}

// bands cover the tiles in order and respect the scratch budget (a single tile may exceed it); segments follow each other and
// complete the parts in order; the items of a band cover every tile's chunk range exactly once
int check_bands_and_items(const CheckJob &job, const Layout &L, const Tuning &tu, const PairPlan &pp, Err &E)
{
    const std::vector<U4> &T = pp.T;
    const uint32_t cpp_ = chunks_per_plane(tu);
    size_t at = 0;
    if (pp.bands.size() != pp.segs.size() || pp.bands.size() != pp.band_items.size()) return E.fail("band bookkeeping sizes differ");
    std::vector<int> part_done(pp.nparts, 0);
    int last_part = -1;
    for (size_t bi = 0; bi < pp.bands.size(); ++bi) {
        const auto &bd = pp.bands[bi];
        if (bd.first != at || bd.second <= bd.first || bd.second > T.size()) return E.fail("band %zu = [%zu,%zu) does not follow %zu", bi, bd.first, bd.second, at);
        at = bd.second;
        if (bd.second - bd.first > 1 && (bd.second - bd.first) * pp.per_tile_bytes > job.cum_budget)
            return E.fail("band %zu needs %llu bytes of C(v), budget %llu", bi, (unsigned long long)((bd.second - bd.first) * pp.per_tile_bytes), (unsigned long long)job.cum_budget);
        size_t sa = bd.first;
        for (const Seg &sg : pp.segs[bi]) {
            if (sg.b != sa || sg.e <= sg.b || sg.e > bd.second) return E.fail("segment [%zu,%zu) of band %zu does not follow %zu", sg.b, sg.e, bi, sa);
            sa = sg.e;
            if (sg.part >= 0) {
                if ((uint32_t)sg.part >= pp.nparts || part_done[sg.part]++ || sg.part != last_part + 1)
                    return E.fail("part %d completed out of order or twice", sg.part);
                last_part = sg.part;
            }
            // every tile of the segment belongs to the part that is current (parts are runs of the WANTED order)
            if (job.plan_parts())
                for (size_t t = sg.b; t < sg.e; ++t) {
                    uint64_t pos0 = ~0ull;  // wanted rows in front of the tile's row block
                    for (size_t k = 0; k < L.wtr.size(); ++k)
                        if (T[t].x >= L.wtr[k].first && T[t].x < L.wtr[k].second) pos0 = L.wtr_w[k] + (uint64_t)(T[t].x - L.wtr[k].first) * kTile;
                    const int cur = last_part + (sg.part >= 0 ? 0 : 1);
                    if (cur < 0 || (size_t)cur + 1 >= L.part_w.size() || pos0 < L.part_w[cur] || pos0 >= L.part_w[cur + 1])
                        return E.fail("tile row %u is not in part %d", T[t].x, cur);
                }
        }
        if (sa != bd.second) return E.fail("segments of band %zu end at %zu, not %zu", bi, sa, bd.second);
        // items of the band cover every tile's chunk range exactly once
        const auto &bi_ = pp.band_items[bi];
        if (band_item_count(tu, pp, bi) != bi_.second - bi_.first) return E.fail("band %zu: band_item_count disagrees with the items built", bi);
        std::vector<std::vector<std::pair<uint32_t, uint32_t>>> per(bd.second - bd.first);
        // overflow fragments (plan.h): the band's LAST band_frags items, each inside one plane, equal in length, at most one
        // round of them; the whole items in front of them a whole number of rounds
        const uint32_t nfr = bi < pp.band_frags.size() ? pp.band_frags[bi] : 0u;
        const uint32_t bri = bi < pp.band_round.size() ? pp.band_round[bi] : 0u;  // the round this band was planned for
        if (bri != tu.round_items && !(tu.small_round_items && bri == tu.small_round_items)) return E.fail("band %zu: round of %u items", bi, bri);
        if (nfr > bi_.second - bi_.first || nfr > bri) return E.fail("band %zu: %u fragments", bi, nfr);
        if (nfr && (!tu.lockstep || (bi_.second - bi_.first - nfr) % bri)) return E.fail("band %zu: fragments behind %zu whole items", bi, bi_.second - bi_.first - nfr);
        for (size_t it = bi_.first; it < bi_.second; ++it) {
            const U4 &I = pp.items[it];
            if (I.x >= per.size() || I.y >= I.z) return E.fail("item %zu is malformed", it);
            const bool frag = it >= bi_.second - nfr;
            if ((I.w != 0) != frag) return E.fail("item %zu: fragment flag %u at the wrong place", it, I.w);
            if (frag && (I.y / cpp_ != (I.z - 1) / cpp_ || I.z - I.y != pp.items[bi_.second - 1].z - pp.items[bi_.second - 1].y))
                return E.fail("fragment %zu spans two planes or differs in length", it);
            per[I.x].emplace_back(I.y, I.z | (frag ? 0x80000000u : 0u));
        }
        for (size_t t = 0; t < per.size(); ++t) {
            std::sort(per[t].begin(), per[t].end());
            uint32_t x = pp.chunks[bd.first + t].x;
            for (size_t k = 0; k < per[t].size(); ++k) {
                auto &pr = per[t][k];
                const bool frag = (pr.second & 0x80000000u) != 0;
                pr.second &= 0x7FFFFFFFu;
                if (pr.first != x) return E.fail("items of tile %zu leave a gap or overlap at chunk %u", t, x);
                // whole items are stored, fragments added: a plane is covered by ONE whole item or by fragments only
                if (!frag && tu.W >= (uint32_t)tu.kc && ((pr.first % cpp_) || (pr.second % cpp_))) return E.fail("an item of tile %zu is not whole planes", t);
                if (frag && (pr.first % cpp_) && !(k > 0 && (per[t][k - 1].second & 0x7FFFFFFFu) == pr.first))
                    return E.fail("a fragment of tile %zu starts inside a plane that fragments do not cover from its start", t);
                x = pr.second;
            }
            if (x != pp.chunks[bd.first + t].y) return E.fail("items of tile %zu end at chunk %u, not %u", t, x, pp.chunks[bd.first + t].y);
        }
    }
    if (at != T.size()) return E.fail("bands end at %zu of %zu tiles", at, T.size());
    return 0;
}

// sparse outer planes: every plane of a tile's range is in the tile's chunk range (check_bands_and_items holds the items to
// pp.chunks) or has exactly one sparse item, never both; a routed plane's sets are inside the cap.
// With the sided route every plane of a tile's range is in exactly one route: the dense remainder [pb + below, pe - above)
// -- one range -- or one sparse item; an item's list block is within its bound, in the item's polarity, for every sketch.
// Then the routes, items and slabs go to the caller that asked for them.
int check_sparse(const CheckJob &job, const Layout &L, const Tuning &tu, const PairPlan &pp, Err &E)
{
    const std::vector<U4> &T = pp.T;
    const SparseCheck *sc = job.sc;
    const uint32_t *keys = job.keys;
    if (pp.sp.size() != T.size() || pp.spb.size() != T.size() || pp.band_sp_items.size() != pp.bands.size()) return E.fail("sparse bookkeeping sizes differ");
    const bool sided_chk = sc && sc->thr && sc->sided != 0 && pp.sided_items > 0;
    const uint32_t cpp_ = chunks_per_plane(tu);
    std::vector<uint8_t> seen_pl;
    size_t sat = 0;
    for (size_t bi = 0; bi < pp.bands.size(); ++bi) {
        const auto &bd = pp.bands[bi];
        const auto &rg = pp.band_sp_items[bi];
        if (rg.first != sat || rg.second < rg.first || rg.second > pp.sp_items.size()) return E.fail("sparse items of band %zu do not follow %zu", bi, sat);
        sat = rg.second;
        seen_pl.assign((bd.second - bd.first) * 64, 0);
        for (size_t k = rg.first; k < rg.second; ++k) {
            const U4 &I = pp.sp_items[k];
            if (I.x >= bd.second - bd.first) return E.fail("sparse item %zu names tile %u of band %zu", k, I.x, bi);
            const size_t t = bd.first + I.x;
            const uint32_t sp = pp.sp[t], spb = pp.spb[t], Ipl = I.y & kSpPlaneMask;
            if (Ipl >= T[t].w || Ipl < T[t].z || (Ipl + sp < T[t].w && Ipl >= T[t].z + spb))
                return E.fail("sparse item %zu: plane %u is not one of the top %u or bottom %u of tile %zu", k, Ipl, sp, spb, t);
            if (T[t].w - T[t].z > 64) return E.fail("tile %zu has %u planes: register values are below 64", t, T[t].w - T[t].z);
            if (seen_pl[I.x * 64 + (Ipl - T[t].z)]++) return E.fail("plane %u of tile %zu has two sparse items", Ipl, t);
            if (I.z >= pp.slabs.size() || I.w >= pp.slabs.size() || pp.slabs[I.z].x != T[t].x || (pp.slabs[I.z].y & kSpPlaneMask) != Ipl ||
                pp.slabs[I.w].x != T[t].y || (pp.slabs[I.w].y & kSpPlaneMask) != Ipl)
                return E.fail("sparse item %zu names the wrong slabs", k);
            const int v = L.pbase + 1 + (int)Ipl;
            if (sided_chk) {
                const bool tr = (I.y & kSpItemTransposed) != 0, la = (I.y & kSpItemListA) != 0, ta = (I.y & kSpItemTabA) != 0;
                if (tr && T[t].x == T[t].y) return E.fail("sparse item %zu: a diagonal tile is transposed", k);
                const U2 &lsl = pp.slabs[tr ? I.w : I.z], &tsl = pp.slabs[tr ? I.z : I.w];
                if (((lsl.y & kSpSlabA) != 0) != la || ((tsl.y & kSpSlabA) != 0) != ta) return E.fail("sparse item %zu: polarities differ from its slabs'", k);
                if (lsl.y & kSpSlabTableOnly) return E.fail("sparse item %zu reads lists from a table-only slab", k);
                if (L.thr_cap != tu.sparse_cap) return E.fail("sparse item %zu planned on thresholds of cap %u at cap %u", k, L.thr_cap, tu.sparse_cap);
                for (uint32_t a = 0; a < kTile; ++a) {
                    const uint64_t sx = (uint64_t)lsl.x * kTile + a;
                    if (sx >= L.ncols) continue;
                    const uint32_t th = sc->thr[L.perm[sx]];
                    if (la ? v > (int)((th >> 8) & 0xFFu) : v < (int)(th & 0xFFu))
                        return E.fail("sparse item %zu: sketch %llu of the list block is outside its bound at v = %d", k, (unsigned long long)L.perm[sx], v);
                }
                continue;
            }
            if (I.y != Ipl || pp.slabs[I.z].y != Ipl || pp.slabs[I.w].y != Ipl) return E.fail("sparse item %zu carries flags without the sided route", k);
            if (sparse_bound(L, T[t].x, v) > tu.sparse_cap || sparse_bound(L, T[t].y, v) > tu.sparse_cap) return E.fail("sparse item %zu: a set may exceed the cap", k);
            // the bound holds for every sketch of the two blocks (what the lists and counters are sized by)
            if (sc && sc->gcnt)
                for (int side = 0; side < 2; ++side)
                    for (uint32_t a = 0; a < kTile; ++a) {
                        const uint64_t sx = (uint64_t)(side ? T[t].y : T[t].x) * kTile + a;
                        if (sx >= L.ncols) continue;
                        const uint32_t key = keys[L.perm[sx]], g = sc->gcnt[L.perm[sx]];
                        const uint32_t own = v >= key_T(key) ? (g & 0xFFFFu) : v == key_T(key) - 1 ? g >> 16 : 65535u;
                        if (own > tu.sparse_cap) return E.fail("sparse item %zu: sketch %llu may hold %u positions", k, (unsigned long long)L.perm[sx], own);
                    }
        }
        for (size_t t = bd.first; t < bd.second; ++t) {
            const uint32_t sp = pp.sp[t], spb = pp.spb[t], np = T[t].w - T[t].z;
            if ((!sided_chk && (sp > 2 || spb)) || sp + spb > np) return E.fail("tile %zu routes %u + %u planes of %u", t, spb, sp, np);
            if (np > 64) return E.fail("tile %zu has %u planes: register values are below 64", t, np);
            for (uint32_t x = 0; x < np; ++x)
                if ((seen_pl[(t - bd.first) * 64 + x] != 0) != (x < spb || x + sp >= np))
                    return E.fail("plane %u of tile %zu: routed and sparse item disagree", T[t].z + x, t);
            if (tu.W >= (uint32_t)tu.kc && (pp.chunks[t].x != (T[t].z + spb) * cpp_ || pp.chunks[t].y != (T[t].w - sp) * cpp_))
                return E.fail("tile %zu: the dense chunk range is not the planes left over", t);
        }
    }
    if (sat != pp.sp_items.size()) return E.fail("sparse items end at %zu of %zu", sat, pp.sp_items.size());
    if (sc && sc->routes) {
        if (T.size() > sc->routes_cap) return E.fail("%zu tiles, room for %llu routes", T.size(), (unsigned long long)sc->routes_cap);
        for (size_t t = 0; t < T.size(); ++t) {
            uint32_t *o = sc->routes + 5 * t;
            o[0] = T[t].x, o[1] = T[t].y, o[2] = T[t].z, o[3] = T[t].w, o[4] = pp.sp[t];
        }
    }
    if (sc && sc->routes6) {
        if (T.size() > sc->routes_cap || pp.sp_items.size() > sc->items_cap || pp.slabs.size() > sc->slabs_cap)
            return E.fail("%zu tiles, %zu items, %zu slabs: no room", T.size(), pp.sp_items.size(), pp.slabs.size());
        for (size_t t = 0; t < T.size(); ++t) {
            uint32_t *o = sc->routes6 + 6 * t;
            o[0] = T[t].x, o[1] = T[t].y, o[2] = T[t].z, o[3] = T[t].w, o[4] = pp.spb[t], o[5] = pp.sp[t];
        }
        for (size_t bi = 0; bi < pp.bands.size(); ++bi)
            for (size_t k = pp.band_sp_items[bi].first; k < pp.band_sp_items[bi].second; ++k) {
                const U4 &I = pp.sp_items[k];
                uint32_t *o = sc->items5 + 5 * k;
                o[0] = (uint32_t)(pp.bands[bi].first + I.x), o[1] = I.y & kSpPlaneMask, o[2] = I.y >> 8, o[3] = I.z, o[4] = I.w;
            }
        for (size_t k = 0; k < pp.slabs.size(); ++k) {
            uint32_t *o = sc->slabs3 + 3 * k;
            o[0] = pp.slabs[k].x, o[1] = pp.slabs[k].y & kSpPlaneMask, o[2] = pp.slabs[k].y >> 8;
        }
    }
    return 0;
}

// every part completes once, and the tile counts the signalling k_finalize waits for add up
int check_parts(const CheckJob &job, const Layout &L, const PairPlan &pp, Err &E)
{
    std::vector<int> part_done(pp.nparts, 0);
    for (const auto &sv : pp.segs)
        for (const Seg &sg : sv)
            if (sg.part >= 0) ++part_done[sg.part];  // (in range: check_bands_and_items)
    for (uint32_t qd = 0; qd < pp.nparts; ++qd)
        if (part_done[qd] != 1) return E.fail("part %u never completes", qd);
    if (pp.nparts) {
        uint64_t tsum = 0;
        if (pp.part_tiles.size() != pp.nparts) return E.fail("part_tiles has %zu entries for %u parts", pp.part_tiles.size(), pp.nparts);
        for (uint32_t c : pp.part_tiles) tsum += c;
        if (tsum != pp.T.size()) return E.fail("the parts hold %llu tiles of %zu", (unsigned long long)tsum, pp.T.size());
    }
    if (job.plan_parts() && pp.nparts + 1 != L.part_w.size()) return E.fail("%u parts planned, layout has %zu", pp.nparts, L.part_w.size() - 1);
    return 0;
}

// the two device lists describe the same tiles
int check_device_lists(const Layout &L, const PairPlan &pp, Err &E)
{
    const std::vector<U4> &T = pp.T;
    std::vector<U4> dt(T.size()), df(T.size());
    emit_tile_lists(L, pp, dt.data(), df.data());
    for (size_t bi = 0; bi < pp.bands.size(); ++bi)
        for (const Seg &sg : pp.segs[bi]) {
            std::vector<uint8_t> used(pp.bands[bi].second - pp.bands[bi].first, 0);
            for (size_t t = sg.b; t < sg.e; ++t) {
                const U4 &f = df[t];
                const uint32_t fw = f.w & 0xFFFFu, fpart = f.w >> 16;  // (C(v) block in the band | the tile's part)
                const size_t src = pp.bands[bi].first + fw;
                if (fw >= used.size() || src < sg.b || src >= sg.e || used[fw]++) return E.fail("finalize list names a C(v) block twice or outside its segment");
                if (pp.nparts) {
                    if (fpart >= pp.nparts || src < pp.part_first[fpart] || src >= pp.part_first[fpart + 1])
                        return E.fail("finalize list entry %zu carries part %u, which does not hold tile %zu", t, fpart, src);
                } else if (fpart) {
                    return E.fail("finalize list entry %zu carries a part without parts", t);
                }
                if (f.x != T[src].x || f.y != T[src].y || (f.z & 0xFFu) != T[src].z || ((f.z >> 8) & 0xFFu) != T[src].w)
                    return E.fail("finalize list entry %zu does not match tile %zu", t, src);
                if (dt[src].x != T[src].x || dt[src].y != T[src].y || dt[src].z != (T[src].z | (T[src].w << 8)))
                    return E.fail("tile list entry %zu is wrong", src);
                const int lo = (int)((f.z >> 16) & 0xFFu), hi = (int)(f.z >> 24);
                if (hi - lo + 1 > sg.hist_bins) return E.fail("segment hist_bins %d too small for tile %zu", sg.hist_bins, src);
            }
            // tile row by tile row inside the segment, columns ascending (the tile rows come in the wanted order: the
            // extra segments' first)
            std::vector<uint32_t> rows_seen;
            for (size_t t = sg.b + 1; t < sg.e; ++t) {
                if (df[t - 1].x == df[t].x) {
                    if (df[t - 1].y >= df[t].y) return E.fail("finalize list of a segment is not row-major at %zu", t);
                } else {
                    rows_seen.push_back(df[t - 1].x);
                    if (std::find(rows_seen.begin(), rows_seen.end(), df[t].x) != rows_seen.end())
                        return E.fail("finalize list of a segment returns to tile row %u at %zu", df[t].x, t);
                }
            }
        }
    return 0;
}

// the stats, as many as the caller has slots for (CheckJob); `any`: something was planned
void fill_stats(const CheckJob &job, const Layout &L, const PairPlan &pp, bool any)
{
    uint64_t full[15] = {0};
    full[5] = L.Npad;
    full[6] = L.P;
    if (any) {
        uint64_t planes_sum = 0;
        for (const U4 &t : pp.T) planes_sum += t.w - t.z;
        full[0] = pp.T.size();
        full[1] = pp.bands.size();
        full[2] = pp.items.size();
        full[3] = pp.nparts;
        full[4] = planes_sum * 100 / pp.T.size();
        // rounds of the lockstep tile kernel over all bands (a band of k items takes ceil(k / its round) rounds)
        for (size_t b = 0; b < pp.band_items.size(); ++b) {
            const uint32_t nfr = pp.band_frags[b], bri = pp.band_round[b];
            full[7] += (pp.band_items[b].second - pp.band_items[b].first - nfr + bri - 1) / bri + (nfr ? 1 : 0);
            full[8] += nfr;
        }
        full[9] = pp.band_round[0];
        full[10] = pp.sp_items.size(), full[11] = pp.slabs.size();
        full[12] = pp.sided_items, full[13] = pp.transposed_items, full[14] = pp.table_slabs;
    }
    // (nothing planned: the slots above the first nine keep what the entry point put there)
    for (int i = 0; i < (any ? std::min(job.stats_slots, 15) : 9); ++i) job.stats[i] = full[i];
}

// the fields every entry point gives
CheckJob base_job(uint64_t n, const uint32_t *keys, int mode, int want_sorted, uint64_t rb, uint64_t re, uint32_t nparts, int want_parts, int p,
                  uint64_t cum_budget)
{
    CheckJob job;
    job.n = n, job.keys = keys, job.mode = mode, job.want_sorted = want_sorted, job.rb = rb, job.re = re;
    job.nparts = nparts, job.want_parts = want_parts, job.p = p, job.cum_budget = cum_budget;
    return job;
}

int plan_check(CheckJob job, char *err, size_t cap)
{
    Err E{err, cap};
    job.resolve();
    if (!job.extra.empty() && !(job.want_sorted && job.mode == 0)) return E.fail("extra segments need a sorted triangle layout");
    Layout L;
    job_layout(job, L);
    uint64_t nw = 0;
    for (auto &w : job.wanted_segments()) nw += w.second - w.first;
    if (job.want_sorted && job.mode == 0 && L.nwanted != nw) return E.fail("nwanted %llu != %llu", (unsigned long long)L.nwanted, (unsigned long long)nw);
    if (job.rowsorted && check_rowsorted(job, L, E)) return -1;
    if (check_layout(job, L, E)) return -1;
    Tuning tu;
    PairQuery q;
    PairPlan pp;
    const bool any = job_plan(job, L, tu, q, pp);
    fill_stats(job, L, pp, false);
    if (!any) {
        const uint64_t wanted = wanted_pairs(job);
        if (wanted) return E.fail("nothing planned although %llu pairs are wanted", (unsigned long long)wanted);
        return 0;
    }
    if (check_coverage(job, L, pp, E) || check_bands_and_items(job, L, tu, pp, E) || check_sparse(job, L, tu, pp, E) || check_parts(job, L, pp, E) ||
        check_device_lists(L, pp, E))
        return -1;
    fill_stats(job, L, pp, true);
    return 0;
}

}  // namespace

extern "C" {

int dshh_plan_check(uint64_t n, const uint32_t *keys, int mode, int want_sorted, uint64_t rb, uint64_t re, uint64_t cb,
                    uint64_t ce, uint32_t nparts, int want_parts, int p, uint64_t cum_budget, int lockstep, int nsplit,
                    int ls_item_chunks, uint64_t *stats, char *err, size_t cap)
{
    CheckJob job = base_job(n, keys, mode, want_sorted, rb, re, nparts, want_parts, p, cum_budget);
    job.cb = cb, job.ce = ce;
    job.lockstep = lockstep, job.nsplit = nsplit, job.ls_item_chunks = ls_item_chunks;
    job.stats = stats, job.stats_slots = 9;
    return plan_check(job, err, cap);
}

// the same check with the tile kernel's round given (a multiple of 256: 256 x the items per workgroup)
int dshh_plan_check_ri(uint64_t n, const uint32_t *keys, int mode, int want_sorted, uint64_t rb, uint64_t re, uint64_t cb,
                       uint64_t ce, uint32_t nparts, int want_parts, int p, uint64_t cum_budget, int lockstep, int nsplit,
                       int ls_item_chunks, uint32_t round_items, uint64_t *stats, char *err, size_t cap)
{
    Err E{err, cap};
    if (round_items == 0 || round_items % 256) return E.fail("round_items %u is not a positive multiple of 256", round_items);
    CheckJob job = base_job(n, keys, mode, want_sorted, rb, re, nparts, want_parts, p, cum_budget);
    job.cb = cb, job.ce = ce;
    job.lockstep = lockstep, job.nsplit = nsplit, job.ls_item_chunks = ls_item_chunks;
    job.round_items = round_items;
    job.stats = stats, job.stats_slots = 10;
    return plan_check(job, err, cap);
}

// the same with the sparse outer planes planned (plan.h, Tuning::sparse_planes): gcnt = the per-sketch counts g0 | g1 << 16
// next to the keys (NULL: none), sparse_planes / sparse_cap the two options.  stats gets twelve slots: [10] sparse items,
// [11] slabs.  routes (or NULL): 5 words per tile -- row block, column block, plane begin, plane end, planes routed sparse.
int dshh_plan_check_sparse(uint64_t n, const uint32_t *keys, const uint32_t *gcnt, int mode, int want_sorted, uint64_t rb, uint64_t re,
                           uint32_t nparts, int want_parts, int p, uint64_t cum_budget, uint32_t round_items, int sparse_planes,
                           uint32_t sparse_cap, uint64_t *stats, uint32_t *routes, uint64_t routes_cap, char *err, size_t cap)
{
    Err E{err, cap};
    if (round_items == 0 || round_items % 256) return E.fail("round_items %u is not a positive multiple of 256", round_items);
    SparseCheck sc;
    sc.gcnt = gcnt;
    sc.planes = sparse_planes;
    sc.cap = sparse_cap;
    sc.routes = routes;
    sc.routes_cap = routes_cap;
    stats[10] = stats[11] = 0;
    CheckJob job = base_job(n, keys, mode, want_sorted, rb, re, nparts, want_parts, p, cum_budget);
    job.round_items = round_items;
    job.sc = &sc;
    job.stats = stats, job.stats_slots = 12;
    return plan_check(job, err, cap);
}

// the same with the sided route planned (plan.h, Tuning::sparse_sided): thr = the per-sketch thresholds vU | vA << 8 at the cap
// thr_cap, sparse_sided the option.  Checks the contract -- every (tile, plane) in exactly one route, the dense remainder one
// range, every item's list block within its bound in the item's polarity -- and returns the plan: stats gets fifteen slots
// ([12] items of the sided route, [13] transposed items, [14] table-only slabs); routes 6 words per tile, items 5 per item
// (tile index, plane, flags, slab of the row block, slab of the column block), slabs 3 per slab (SparseCheck above).
int dshh_plan_check_sparse_sided(uint64_t n, const uint32_t *keys, const uint32_t *gcnt, const uint32_t *thr, uint32_t thr_cap, int mode,
                                 int want_sorted, uint64_t rb, uint64_t re, uint32_t nparts, int want_parts, int p, uint64_t cum_budget,
                                 uint32_t round_items, int sparse_planes, int sparse_sided, uint32_t sparse_cap, uint64_t *stats, uint32_t *routes,
                                 uint64_t routes_cap, uint32_t *items, uint64_t items_cap, uint32_t *slabs, uint64_t slabs_cap, char *err, size_t cap)
{
    Err E{err, cap};
    if (round_items == 0 || round_items % 256) return E.fail("round_items %u is not a positive multiple of 256", round_items);
    if (!routes || !items || !slabs) return E.fail("routes, items and slabs are wanted");
    SparseCheck sc;
    sc.gcnt = gcnt;
    sc.planes = sparse_planes;
    sc.cap = sparse_cap;
    sc.thr = thr;
    sc.thr_cap = thr_cap;
    sc.sided = sparse_sided;
    sc.routes6 = routes, sc.routes_cap = routes_cap;
    sc.items5 = items, sc.items_cap = items_cap;
    sc.slabs3 = slabs, sc.slabs_cap = slabs_cap;
    for (int i = 10; i < 15; ++i) stats[i] = 0;
    CheckJob job = base_job(n, keys, mode, want_sorted, rb, re, nparts, want_parts, p, cum_budget);
    job.round_items = round_items;
    job.sc = &sc;
    job.stats = stats, job.stats_slots = 15;
    return plan_check(job, err, cap);
}

// the rows of ONE rank of a row-set table (plan.h): main range + extra segments, row-sorted parts (rowsorted != 0: what a
// source rank of the exchange computes) or one part in final order (the destination)
int dshh_plan_check_rowset(uint64_t n, const uint32_t *keys, const uint64_t *tab, uint32_t rank, int rowsorted, uint32_t nparts, int p,
                           uint64_t cum_budget, uint64_t *stats, char *err, size_t cap)
{
    Err E{err, cap};
    RowSets rs;
    if (const char *why = parse_rowsets(tab, n, rs)) return E.fail("%s", why);
    if (rank >= rs.world) return E.fail("rank %u of %u", rank, rs.world);
    uint64_t rb, re;
    std::vector<uint64_t> extra;
    rs.rank_rows(rank, rb, re, extra);
    for (int i = 0; i < 9; ++i) stats[i] = 0;
    if (rb >= re) return 0;
    CheckJob job = base_job(n, keys, rowsorted ? 3 : 0, 1, rb, re, rowsorted ? nparts : 1, 1, p, cum_budget);
    job.extra = extra;
    job.stats = stats, job.stats_slots = 9;
    return plan_check(job, err, cap);
}

}  // extern "C"

namespace {

// ---- dshh_plan_digest: what a layout and a plan ARE, section by section (tests/test_plan_digest.py) ---------------------
// the sections, in the order their digests are written
const char *const kDigestNames =
    "perm,parts,part_w,part_pos,rowoff,rowoff_w,wtr,wtr_w,blk_T,blk_lo,blk_L,blk_hi,blk_g0,blk_g1,blk_vU,blk_vA,"
    "Npad,ncols,nwanted,pbase,P,vlo,vhi,whole,rowsorted,thr_cap,"
    "T,bands,band_items,band_round,band_frags,segs,items,rank,chunks,part_tiles,part_first,sp,spb,sp_items,band_sp_items,slabs,"
    "per_tile_bytes,max_band,nparts,sided_items,transposed_items,table_slabs,"
    "dev_tiles,dev_ftiles,band_item_count";
constexpr uint32_t kDigestSections = 51;

// 64-bit FNV-1a over the values of a section, every value as eight little-endian bytes (so that no padding and no host
// type width enters a digest)
struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void add(uint64_t v)
    {
        for (int i = 0; i < 8; ++i) h = (h ^ ((v >> (8 * i)) & 0xFFu)) * 1099511628211ull;
    }
    void add(const U4 &v) { add(v.x), add(v.y), add(v.z), add(v.w); }
    void add(const U2 &v) { add(v.x), add(v.y); }
    template <class A, class B>
    void add(const std::pair<A, B> &v) { add((uint64_t)v.first), add((uint64_t)v.second); }
    void add(const Seg &s) { add((uint64_t)s.b), add((uint64_t)s.e), add((uint64_t)(int64_t)s.part), add((uint64_t)(int64_t)s.hist_bins); }
};

struct DigestOut {
    uint64_t *out;
    uint32_t at = 0;
    template <class T>
    void vec(const std::vector<T> &v)
    {
        Fnv f;
        for (const T &x : v) f.add(x);
        out[at++] = f.h;
    }
    void scalar(uint64_t v)
    {
        Fnv f;
        f.add(v);
        out[at++] = f.h;
    }
};

// the digests of a layout and its plan (`any`: build_pairs planned something), and which branches of the planner the case reached
uint64_t digest_plan(const Layout &L, const Tuning &tu, const PairQuery &q, const PairPlan &pp, bool any, uint64_t *out)
{
    DigestOut D{out};
    D.vec(L.perm), D.vec(L.parts), D.vec(L.part_w), D.vec(L.part_pos), D.vec(L.rowoff), D.vec(L.rowoff_w), D.vec(L.wtr), D.vec(L.wtr_w);
    D.vec(L.blk_T), D.vec(L.blk_lo), D.vec(L.blk_L), D.vec(L.blk_hi), D.vec(L.blk_g0), D.vec(L.blk_g1), D.vec(L.blk_vU), D.vec(L.blk_vA);
    D.scalar(L.Npad), D.scalar(L.ncols), D.scalar(L.nwanted), D.scalar((uint64_t)(int64_t)L.pbase), D.scalar(L.P);
    D.scalar((uint64_t)(int64_t)L.vlo), D.scalar((uint64_t)(int64_t)L.vhi), D.scalar(L.whole), D.scalar((uint64_t)L.rowsorted), D.scalar(L.thr_cap);
    D.vec(pp.T), D.vec(pp.bands), D.vec(pp.band_items), D.vec(pp.band_round), D.vec(pp.band_frags);
    {
        Fnv f;
        for (const auto &sv : pp.segs) {
            f.add((uint64_t)sv.size());
            for (const Seg &s : sv) f.add(s);
        }
        D.out[D.at++] = f.h;
    }
    D.vec(pp.items), D.vec(pp.rank), D.vec(pp.chunks), D.vec(pp.part_tiles), D.vec(pp.part_first), D.vec(pp.sp), D.vec(pp.spb);
    D.vec(pp.sp_items), D.vec(pp.band_sp_items), D.vec(pp.slabs);
    D.scalar(pp.per_tile_bytes), D.scalar(pp.max_band), D.scalar(pp.nparts), D.scalar(pp.sided_items), D.scalar(pp.transposed_items);
    D.scalar(pp.table_slabs);
    std::vector<U4> dt(any ? pp.T.size() : 0), df(dt.size());
    std::vector<uint64_t> counts;
    if (any) {
        emit_tile_lists(L, pp, dt.data(), df.data());
        for (size_t bi = 0; bi < pp.bands.size(); ++bi) counts.push_back(band_item_count(tu, pp, bi));
    }
    D.vec(dt), D.vec(df), D.vec(counts);
    // ---- the feature word
    uint64_t F = 0;
    auto bit = [&](int b, bool on) { F |= on ? 1ull << b : 0; };
    bit(5, pp.nparts > 1), bit(6, L.rowsorted != 0), bit(7, L.rowsorted && L.parts.size() == 3), bit(8, !L.extra.empty());
    bit(9, q.rect != 0), bit(10, q.sorted_rows != 0), bit(11, !L.sorted), bit(12, tu.W < (uint32_t)tu.kc), bit(13, tu.nsplit > 0);
    bit(14, !tu.lockstep), bit(20, tu.cum_bytes == 4);
    if (!any) return F;
    bit(0, pp.bands.size() > 1);
    const uint64_t max_tiles = std::min<uint64_t>(65536, std::max<uint64_t>(1, tu.cum_budget / std::max<uint64_t>(pp.per_tile_bytes, 1)));
    for (size_t bi = 0; bi + 1 < pp.bands.size(); ++bi) {  // why a band ends before the tiles do
        const size_t e = pp.bands[bi].second;
        bool by_part = false;
        for (uint32_t qd = 0; qd < pp.nparts; ++qd) by_part |= pp.part_first[qd + 1] == e && pp.part_tiles[qd] >= tu.part_band_tiles;
        bit(1, by_part);
        bit(2, !by_part && e - pp.bands[bi].first < max_tiles);
    }
    for (size_t bi = 0; bi < pp.bands.size(); ++bi) {
        bit(3, pp.band_frags[bi] > 0);
        bit(4, tu.small_round_items && tu.small_round_items < tu.round_items && pp.band_round[bi] == tu.small_round_items);
    }
    bit(15, pp.sp_items.size() > pp.sided_items), bit(16, pp.sided_items > 0), bit(17, pp.transposed_items > 0), bit(18, pp.table_slabs > 0);
    for (uint8_t b : pp.spb) bit(19, b > 0);
    return F;
}

}  // namespace

extern "C" {

// The characterization hook: layout and plan built exactly as the checks above build them (the inputs of
// dshh_plan_check_sparse_sided and, as dshh_plan_check has them, cb, ce, lockstep, nsplit, ls_item_chunks; round_items 0 =
// the planner's default; extra = n_extra words {b0, e0, ...}), nothing checked.  digests gets one 64-bit FNV-1a value per
// section of dshh_plan_digest_names() (comma-separated, in order), *features which branches the case reached: bit 0 more
// than one band, 1 a band cut by a large part, 2 a tail cut, 3 overflow fragments, 4 a band at small_round_items, 5 parts
// > 1, 6 row-sorted, 7 a two-run row-sorted range, 8 extra segments, 9 rectangle, 10 sorted_rows, 11 identity layout,
// 12 W < kc, 13 nsplit > 0, 14 not lockstep, 15 two-plane items, 16 sided items, 17 transposed items, 18 table-only slabs,
// 19 planes routed from the bottom of a range, 20 cum_bytes = 4.  Returns the number of sections, -1 on a bad argument.
const char *dshh_plan_digest_names(void) { return kDigestNames; }

int dshh_plan_digest(uint64_t n, const uint32_t *keys, const uint32_t *gcnt, const uint32_t *thr, uint32_t thr_cap, int mode, int want_sorted,
                     uint64_t rb, uint64_t re, uint64_t cb, uint64_t ce, uint32_t nparts, int want_parts, int p, uint64_t cum_budget, int lockstep,
                     int nsplit, int ls_item_chunks, uint32_t round_items, int sparse_planes, int sparse_sided, uint32_t sparse_cap,
                     const uint64_t *extra, uint32_t n_extra, uint64_t *digests, uint32_t digests_cap, uint64_t *features, char *err, size_t cap)
{
    Err E{err, cap};
    if (round_items % 256) return E.fail("round_items %u is not a multiple of 256", round_items);
    if (!digests || !features || digests_cap < kDigestSections || n_extra % 2) return E.fail("digests, features and whole extra segments are wanted");
    SparseCheck sc;
    sc.gcnt = gcnt;
    sc.planes = sparse_planes;
    sc.cap = sparse_cap;
    sc.thr = thr;
    sc.thr_cap = thr_cap;
    sc.sided = sparse_sided;
    CheckJob job = base_job(n, keys, mode, want_sorted, rb, re, nparts, want_parts, p, cum_budget);
    job.cb = cb, job.ce = ce;
    job.lockstep = lockstep, job.nsplit = nsplit, job.ls_item_chunks = ls_item_chunks;
    job.extra.assign(extra, extra + (extra ? n_extra : 0));
    job.round_items = round_items;
    job.sc = &sc;
    job.resolve();
    if (!job.extra.empty() && !(job.want_sorted && job.mode == 0)) return E.fail("extra segments need a sorted triangle layout");
    Layout L;
    job_layout(job, L);
    Tuning tu;
    PairQuery q;
    PairPlan pp;
    const bool any = job_plan(job, L, tu, q, pp);
    *features = digest_plan(L, tu, q, pp, any, digests);
    return (int)kDigestSections;
}

// The sparse items of a plan as the device gets them (read-only; tests/test_sparse_order.py, tests/test_sparse_emit.py): the
// layout and plan of a triangle job built as dshh_plan_check_sparse_sided builds them, with Tuning::sparse_max_slabs given
// (0: the planner's default) and, two_step != 0, through build_tiles + emit_sparse_items + build_band_items in the order
// engine.hip calls them instead of build_pairs.  Nothing is checked.  tiles6: per tile {row block, column block, plane begin,
// plane end, planes routed below, planes routed above} in launch order; bands4: per band {first tile, end tile, first
// sparse item, end sparse item}; items4: per sparse item, in LAUNCH order, {tile index in its band, plane | flags << 8
// (plan.h, kSpItem*), slab of the row block, slab of the column block}; slabs2: per slab {block, plane | flags << 8
// (kSpSlab*)}; chunks2: per tile its dense chunk range.  counts: [0] tiles, [1] bands, [2] sparse items, [3] slabs,
// [4] items of the sided route, [5] transposed items, [6] table-only slabs, [7] dense items, [8] the blocks of the layout
// (NT).  Returns 0; -1 on a bad argument or when a list does not fit its cap (counts are set then too).
int dshh_plan_sparse_items(uint64_t n, const uint32_t *keys, const uint32_t *gcnt, const uint32_t *thr, uint32_t thr_cap, uint64_t rb, uint64_t re,
                           uint32_t nparts, int want_parts, int p, uint64_t cum_budget, uint32_t round_items, int sparse_planes, int sparse_sided,
                           uint32_t sparse_cap, uint32_t sparse_max_slabs, int two_step, uint64_t *counts, uint32_t *tiles6, uint64_t tiles_cap,
                           uint64_t *bands4, uint64_t bands_cap, uint32_t *items4, uint64_t items_cap, uint32_t *slabs2, uint64_t slabs_cap,
                           uint32_t *chunks2, char *err, size_t cap)
{
    Err E{err, cap};
    if (round_items == 0 || round_items % 256) return E.fail("round_items %u is not a positive multiple of 256", round_items);
    if (!counts || !tiles6 || !bands4 || !items4 || !slabs2 || !chunks2) return E.fail("every list is wanted");
    SparseCheck sc;
    sc.gcnt = gcnt;
    sc.planes = sparse_planes;
    sc.cap = sparse_cap;
    sc.thr = thr;
    sc.thr_cap = thr_cap;
    sc.sided = sparse_sided;
    sc.max_slabs = sparse_max_slabs;
    CheckJob job = base_job(n, keys, 0, 1, rb, re, nparts, want_parts, p, cum_budget);
    job.round_items = round_items;
    job.sc = &sc;
    job.resolve();
    Layout L;
    job_layout(job, L);
    Tuning tu;
    PairQuery q;
    PairPlan pp;
    for (int i = 0; i < 9; ++i) counts[i] = 0;
    counts[8] = L.Npad / kTile;
    if (!job_plan(job, L, tu, q, pp, two_step != 0)) return 0;
    counts[0] = pp.T.size(), counts[1] = pp.bands.size(), counts[2] = pp.sp_items.size(), counts[3] = pp.slabs.size();
    counts[4] = pp.sided_items, counts[5] = pp.transposed_items, counts[6] = pp.table_slabs, counts[7] = pp.items.size();
    if (pp.T.size() > tiles_cap || pp.bands.size() > bands_cap || pp.sp_items.size() > items_cap || pp.slabs.size() > slabs_cap)
        return E.fail("%zu tiles, %zu bands, %zu items, %zu slabs: no room", pp.T.size(), pp.bands.size(), pp.sp_items.size(), pp.slabs.size());
    for (size_t t = 0; t < pp.T.size(); ++t) {
        uint32_t *o = tiles6 + 6 * t;
        o[0] = pp.T[t].x, o[1] = pp.T[t].y, o[2] = pp.T[t].z, o[3] = pp.T[t].w, o[4] = pp.spb[t], o[5] = pp.sp[t];
        chunks2[2 * t] = pp.chunks[t].x, chunks2[2 * t + 1] = pp.chunks[t].y;
    }
    for (size_t bi = 0; bi < pp.bands.size(); ++bi) {
        uint64_t *o = bands4 + 4 * bi;
        o[0] = pp.bands[bi].first, o[1] = pp.bands[bi].second, o[2] = pp.band_sp_items[bi].first, o[3] = pp.band_sp_items[bi].second;
    }
    for (size_t k = 0; k < pp.sp_items.size(); ++k) {
        uint32_t *o = items4 + 4 * k;
        o[0] = pp.sp_items[k].x, o[1] = pp.sp_items[k].y, o[2] = pp.sp_items[k].z, o[3] = pp.sp_items[k].w;
    }
    for (size_t k = 0; k < pp.slabs.size(); ++k) slabs2[2 * k] = pp.slabs[k].x, slabs2[2 * k + 1] = pp.slabs[k].y;
    return 0;
}

// the table stagings of one launch of the LDS placement of the sparse counting kernel (plan::sparse_table_fills): items4 = n
// items of four words {tile, plane | flags << 8 (plan.h, kSpItem*), slab of the row block, slab of the column block}, in
// launch order; run as the option sparse_run in effect (tests/test_sparse_runs_model.py)
uint64_t dshh_sparse_table_fills(const uint32_t *items4, uint64_t n, uint32_t run)
{
    static_assert(sizeof(U4) == 4 * sizeof(uint32_t), "an item is four words");
    return sparse_table_fills(reinterpret_cast<const U4 *>(items4), (size_t)n, run);
}

// first row of the second run of a row-sorted range (plan::rowsorted_split), re when the range stays one run
uint64_t dshh_rowsorted_split(uint64_t n, uint64_t rb, uint64_t re) { return rowsorted_split(n, rb, re); }

// the band walk of bands.h (plan::tri_band_end, plan::rect_band_rows) over the rows [rb, re): of the triangle of n sketches
// (ncols == 0; re is cut to n), or of a rectangle of ncols > 0 columns.  bounds[0] = rb, bounds[q + 1] = the end of band q.
// Returns the number of bands (0 for an empty range), or -1 when they do not fit cap boundaries (tests/test_band_plan.py).
int64_t dshh_threshold_bands(uint64_t n, uint64_t rb, uint64_t re, uint64_t ncols, uint64_t band_bytes, uint64_t row_cap,
                             uint64_t *bounds, uint64_t cap)
{
    const uint64_t band_floats = std::max<uint64_t>(band_bytes / sizeof(float), 1);
    if (!ncols && re > n) re = n;
    uint64_t nb = 0;
    if (cap) bounds[0] = rb;
    for (uint64_t b0 = rb; b0 < re;) {
        b0 = ncols ? std::min<uint64_t>(re, b0 + rect_band_rows(ncols, band_floats)) : tri_band_end(n, b0, re, band_floats, row_cap);
        if (++nb >= cap) return -1;
        bounds[nb] = b0;
    }
    return (int64_t)nb;
}

// the grid of k_hist (plan::hist_grid) and the trips of a workgroup's waves it implies (tests/test_hist_ref.py)
uint64_t dshh_hist_grid(uint64_t units, uint64_t lds_bytes, uint32_t cus, uint64_t *iters)
{
    const uint64_t grid = hist_grid(units, lds_bytes, cus);
    if (iters) *iters = units / (4 * grid) + (units % (4 * grid) ? 1 : 0);
    return grid;
}

// the bands of dsh_greedy_threshold* (the loop of greedy.hip: plan::tri_band_end up to row n, the empty last row left out):
// bounds[0] = 0, bounds[q + 1] = the end of band q, for the triangle of n sketches.  Returns the number of bands (0 for
// n < 2), or -1 when they do not fit cap boundaries (tests/test_greedy_plan.py).
int64_t dshh_greedy_bands(uint64_t n, uint64_t band_bytes, uint64_t row_cap, uint64_t *bounds, uint64_t cap)
{
    const uint64_t band_floats = std::max<uint64_t>(band_bytes / sizeof(float), 1);
    uint64_t nb = 0;
    if (cap) bounds[0] = 0;
    for (uint64_t b0 = 0; b0 + 1 < n;) {
        b0 = tri_band_end(n, b0, n, band_floats, row_cap);
        if (++nb >= cap) return -1;
        bounds[nb] = b0;
    }
    return (int64_t)nb;
}

// the bands of old rows of dsh_greedy_extend* (plan::greedy_old_band, the first loop of greedy_extend.hip) for m old slots
// of n: bounds[2 q], bounds[2 q + 1] = band q.  Returns the number of bands, or -1 when they do not fit cap words or m > n
// (tests/test_greedy_extend_plan.py).
int64_t dshh_greedy_extend_bands(const uint32_t *labels_in, uint64_t m, uint64_t n, uint64_t band_bytes, uint64_t *bounds, uint64_t cap)
{
    if (m > n) return -1;
    const uint64_t band_floats = std::max<uint64_t>(band_bytes / sizeof(float), 1);
    uint64_t nb = 0, b0 = 0, b1 = 0;
    for (uint64_t from = 0; greedy_old_band(labels_in, m, n - m, from, band_floats, b0, b1); from = b1) {
        if (2 * nb + 2 > cap) return -1;
        bounds[2 * nb] = b0;
        bounds[2 * nb + 1] = b1;
        ++nb;
    }
    return (int64_t)nb;
}

// the union-find of the threshold clusters (../uf.h, the code the device kernels compile) run sequentially: labels_out[x] =
// the smallest node of x's component in the graph of the n_edges edges (lhs[e], rhs[e]).  Returns 0, -1 for an edge that
// names a node >= n, and the step-bound code (1 find, 2 hook) when a loop overran step_cap -- the give-up path, which the
// device kernels must never reach, is tested here (tests/test_cluster_host.py).
int dsh_plan_uf_labels(uint64_t n, const uint32_t *lhs, const uint32_t *rhs, uint64_t n_edges, uint32_t step_cap, uint32_t *labels_out)
{
    if (n > 0xFFFFFFFFull) return -1;
    std::vector<uint32_t> parent(n);
    for (uint64_t x = 0; x < n; ++x) parent[x] = (uint32_t)x;
    for (uint64_t e = 0; e < n_edges; ++e) {
        if (lhs[e] >= n || rhs[e] >= n) return -1;
        uint32_t why = 0;
        if (uf_unite<UfPlain>(parent.data(), lhs[e], rhs[e], step_cap, &why) == kUfOverrun) return (int)why;
    }
    for (uint64_t x = 0; x < n; ++x) {
        const uint32_t l = uf_find<UfPlain>(parent.data(), (uint32_t)x, step_cap);
        if (l == kUfOverrun) return (int)kUfErrFind;
        labels_out[x] = l;
    }
    return 0;
}

}  // extern "C"

namespace {

template <int L>
int linkage_labels(uint64_t n, const float *tri, const LkThr &thr, uint32_t *labels, uint32_t step_cap)
{
    typedef typename LkCell<L>::T T;
    const uint32_t m = (uint32_t)n;
    std::vector<T> cells((size_t)m * m, T(0)), nnv(m);
    std::vector<uint32_t> alive(m), size(m), nn(m), root(m);
    for (uint32_t i = 0; i < m; ++i)
        for (uint32_t j = i + 1; j < m; ++j)
            cells[(size_t)i * m + j] = cells[(size_t)j * m + i] = lk_cell<L>(tri[tri_index(n, i, j)], thr.descending);
    const uint32_t rc = lk_run_seq<L>(m, cells.data(), alive.data(), size.data(), nn.data(), nnv.data(), root.data(), thr, step_cap, m + 1);
    for (uint32_t i = 0; i < m; ++i) labels[i] = root[i];
    return (int)rc;
}

}  // namespace

extern "C" {

// the linkage clusters at a threshold (../linkage.h, the step logic the device kernel compiles) run sequentially with the
// whole collection as ONE component: labels[x] = the smallest slot of x's final cluster for the n (n - 1) / 2 values of tri
// (dsh_tri_index order).  Returns 0, -1 for a bad argument (an unknown linkage, n above 2^16, AVERAGE with |t| >= 2), and the
// give-up code (1) when the merges overran step_cap -- the path the device kernel must never reach
// (tests/test_linkage_host.py).  A NaN threshold gives n singletons.
int dsh_plan_linkage_labels(uint64_t n, const float *tri, int descending, float threshold, int linkage, uint32_t *labels,
                            uint64_t *n_clusters, uint32_t step_cap)
{
    if (n > 65536 || linkage < kLkSingle || linkage > kLkAverage || (n && !labels) || (n > 1 && !tri)) return -1;
    if (linkage == kLkAverage && threshold == threshold && !(fabsf(threshold) < 2.f)) return -1;
    int rc = 0;
    if (threshold != threshold) {
        for (uint64_t x = 0; x < n; ++x) labels[x] = (uint32_t)x;
    } else {
        const LkThr thr = lk_threshold(threshold, descending ? 1 : 0);
        rc = linkage == kLkSingle     ? linkage_labels<kLkSingle>(n, tri, thr, labels, step_cap)
             : linkage == kLkComplete ? linkage_labels<kLkComplete>(n, tri, thr, labels, step_cap)
                                      : linkage_labels<kLkAverage>(n, tri, thr, labels, step_cap);
    }
    if (n_clusters) {
        *n_clusters = 0;
        for (uint64_t x = 0; x < n; ++x) *n_clusters += labels[x] == x;
    }
    return rc;
}

// the loose float threshold of the AVERAGE partition (lk_loose_threshold) and q(v), for the CPU tests
float dsh_plan_linkage_loose(float threshold, int descending) { return lk_loose_threshold(threshold, descending ? 1 : 0); }
int64_t dsh_plan_linkage_q(float v) { return lk_q(v); }

// the minimum spanning tree of the pair values (../mst.h, the step logic the device kernels compile) run sequentially over the
// n (n - 1) / 2 values of tri (dsh_tri_index order): the edges sorted best first as dsh_mst_tri returns them, labels (or NULL) =
// the smallest node of x's component, *rounds = the rounds that emitted.  Returns 0, -1 for a bad argument, and the give-up code
// (3) when more than round_cap rounds emitted -- the path the device build must never reach (tests/test_mst_host.py).
int dsh_plan_mst(uint64_t n, const float *tri, int descending, float cutoff, uint32_t round_cap, uint32_t *lhs, uint32_t *rhs, float *val,
                 uint64_t *n_edges, uint32_t *labels, uint32_t *rounds)
{
    if (n > 65536 || !n_edges || !rounds || (n > 1 && (!tri || !lhs || !rhs || !val))) return -1;
    std::vector<uint32_t> parent;
    std::vector<MstEdge> e;
    *n_edges = 0;
    const uint32_t rc = mst_run_seq(n, tri, descending ? 1 : 0, cutoff, round_cap, parent, e, rounds);
    if (rc) return (int)rc;
    if (!e.empty()) mst_sorted_out(e, descending ? 1 : 0, lhs, rhs, val);
    *n_edges = e.size();
    if (labels)
        for (uint64_t x = 0; x < n; ++x) labels[x] = uf_find<UfPlain>(parent.data(), (uint32_t)x, (uint32_t)n + 1);
    return 0;
}

}  // extern "C"

namespace {

template <class T>
bool hand_back(const std::vector<T> &v, void *buf, uint64_t &count)
{
    const uint64_t cap = count;
    count = v.size();
    if (!buf) return true;
    if (cap < v.size()) return false;
    if (!v.empty()) std::memcpy(buf, v.data(), v.size() * sizeof(T));
    return true;
}

}  // namespace

extern "C" {

// The host arithmetic of dsh_sketch_fastx_records (../sketch_plan.h), for tests/test_fastx_records_plan.py:
//   dshh_fastx_tail_records   the records to add to a file's markers (-1, 0, +1)
//   dshh_fastx_line_start     the first byte of the line that holds file[pos]
//   dshh_fastx_record_offsets off[n + 1] from the markers' decoded positions and the file's decoded end
int dshh_fastx_tail_records(const uint8_t *file, uint64_t len, uint32_t fmt, uint32_t end_line)
{
    return fastx_tail_records(file, len, fmt, end_line);
}
uint64_t dshh_fastx_line_start(const uint8_t *file, uint64_t pos) { return fastx_line_start(file, pos); }
void dshh_fastx_record_offsets(const uint64_t *dpos, uint64_t markers, uint64_t n, uint64_t end, uint64_t *off)
{
    std::vector<uint64_t> v;
    fastx_record_offsets(dpos, markers, n, end, v);
    std::copy(v.begin(), v.end(), off);
}


// the sketch path's planners (../sketch_plan.h) on a caller's offsets off[n + 1], as sketch.hip runs them behind its checks
// (tests/test_sketch_plan.py).  kind 0: plan_genomes -> list 0 = SketchWork.  kind 1: plan_records -> lists RecRun, RecSeg, rows to
// clear (uint32), SketchWork; info[1] = 1 where the records kernel takes the call (0: all n rows are cleared at once, every record
// is a genome).  kind 2: plan_fastx -> lists FastxGenome, FastxChunk, from the first byte and the raw length of every genome's
// file (the planner reads nothing else of the raw bytes).  counts[4] gets the lists' lengths in elements; with bufs == NULL that
// is all, else bufs[i] (where not NULL) has room for counts[i] elements on entry and gets list i.  Returns 0, -1 for arguments
// sketch.hip's check refuses (offsets not monotone, slots beyond 2^32) or unusable here, -2 for a buffer too small, and a FASTX
// refusal's code (kFastxPlan*) with info[0] = the genome.
int dshh_sketch_plan(int kind, const uint64_t *off, uint32_t n, uint64_t first_slot, int k, int p, const uint8_t *first_byte,
                     const uint64_t *raw_len, void *const *bufs, uint64_t *counts, uint32_t *info)
{
    if (!off || !counts || !info || kind < 0 || kind > 2 || first_slot + n > 0xFFFFFFFFull) return -1;
    info[0] = info[1] = 0;
    void *const none[4] = {nullptr, nullptr, nullptr, nullptr};
    if (!bufs) bufs = none;
    bool fits = true;
    if (kind == 2) {
        // (a genome's region may end before the next begins for the planner, which refuses it: no monotone check in front)
        if (!raw_len || !first_byte) return -1;
        uint64_t hi = 0;
        for (uint32_t g = 0; g <= n; ++g) hi = std::max(hi, off[g]);
        if (hi >= (1ull << 28)) return -1;  // the raw buffer is made here
        std::vector<uint8_t> raw(hi + 1, 0);
        for (uint32_t g = 0; g < n; ++g) raw[off[g]] = first_byte[g];
        std::vector<FastxGenome> gen;
        std::vector<FastxChunk> chunks;
        const int rc = plan_fastx(raw.data(), off, raw_len, n, gen, chunks, &info[0]);
        if (rc) return rc;
        info[0] = 0;
        fits = hand_back(gen, bufs[0], counts[0]);
        fits = hand_back(chunks, bufs[1], counts[1]) && fits;
        counts[2] = counts[3] = 0;
        return fits ? 0 : -2;
    }
    for (uint32_t g = 0; g < n; ++g)
        if (off[g + 1] < off[g]) return -1;
    std::vector<SketchWork> work;
    if (kind == 0) {
        plan_genomes(off, n, first_slot, k, p, work);
        fits = hand_back(work, bufs[0], counts[0]);
        counts[1] = counts[2] = counts[3] = 0;
        return fits ? 0 : -2;
    }
    std::vector<RecRun> runs;
    std::vector<RecSeg> segs;
    std::vector<uint32_t> zero;
    info[1] = plan_records(off, n, first_slot, k, p, runs, segs, zero, work) ? 1 : 0;
    fits = hand_back(runs, bufs[0], counts[0]);
    fits = hand_back(segs, bufs[1], counts[1]) && fits;
    fits = hand_back(zero, bufs[2], counts[2]) && fits;
    fits = hand_back(work, bufs[3], counts[3]) && fits;
    return fits ? 0 : -2;
}

}  // extern "C"

#include "../curve_plan.h"

extern "C" {

// the planner of dsh_union_curve* (../curve_plan.h) as curve.hip runs it (tests/test_curve_plan.py).  info[5] = S, segments per
// order, orders per batch, scratch bytes of one order, scratch bytes of a batch.  bounds (or NULL) has room for `cap` words and
// gets the segments' begins and the end of the order: nseg + 1 words.  Returns 0, -1 for unusable arguments, -2 for a buffer too small.
int dshh_curve_plan(uint64_t n_orders, uint64_t len, int p, uint64_t budget, uint64_t forced_S, uint64_t *info, uint64_t *bounds, uint64_t cap)
{
    if (!info || p < 4 || p > 24) return -1;
    const dsh::curve::Plan pl = dsh::curve::plan(n_orders, len, p, budget, forced_S);
    info[0] = pl.S, info[1] = pl.nseg, info[2] = pl.batch, info[3] = pl.order_bytes, info[4] = pl.scratch_bytes();
    if (!bounds) return 0;
    if (cap < pl.nseg + 1) return -2;
    for (uint64_t s = 0; s <= pl.nseg; ++s) bounds[s] = pl.begin(s, len);
    return 0;
}

}  // extern "C"

#include "../exchange_plan.h"

extern "C" {

// the planning of dsh_exchange_collect_async (../exchange_plan.h) for ONE calling rank of the row-set table `tab`, as
// exchange.hip runs it (tests/test_exchange_plan.py): the modes (fine != 0: the caller cut finely, as a rank whose parts
// are signalled does), the tables of the row-sorted ranks the caller knows -- the destination derives every source's from
// the keys, a source takes its own from its layout, built here as engine.hip builds it -- and the schedule.  The lists:
//   0 total u64[world] | 1 messages u64[M * world][2] {first, cnt} | 2 post u8[M] | 3 gate u32[M] | 4 part_end u64[] |
//   5 stage_off u64[world] | 6 tab_off u64[world] | 7 entries u64[][4] {src, pos0, row0, nrows} | 8 round_ent u32[M + 1] |
//   9 round_rows u32[M] | 10 rowoff u64, the known ranks' one behind the other in rank order | 11 order u32, the same |
//   12 modes u32[world][3] {rowsorted, parts, parts asked for} | 13 the calling rank's cut u64[] (XMode::cut)
// info[3] = stage_total, ent_off, tab_bytes.  counts[14] gets the lists' lengths in elements; with bufs == NULL that is all,
// else bufs[i] (where not NULL) has room for counts[i] elements on entry and gets list i.  Returns 0, -1 for unusable
// arguments, -2 for a buffer too small.
int dshh_exchange_plan(uint64_t n, const uint32_t *keys, const uint64_t *tab, uint32_t nparts, int dst, int rank, int fine, void *const *bufs,
                       uint64_t *counts, uint64_t *info)
{
    RowSets rs;
    if (!keys || !tab || !counts || !info || nparts == 0 || parse_rowsets(tab, n, rs) || dst < 0 || (uint32_t)dst >= rs.world || rank < 0 ||
        (uint32_t)rank >= rs.world)
        return -1;
    const std::vector<xplan::XMode> modes = xplan::xmodes(n, rs, nparts, dst, fine ? rank : -1);
    std::vector<std::vector<uint64_t>> rowoff(rs.world);
    std::vector<std::vector<uint32_t>> order(rs.world);
    std::vector<uint32_t> scratch;
    for (uint32_t r = 0; r < rs.world; ++r) {
        const xplan::XMode &m = modes[r];
        if ((int)r == dst || !m.rowsorted) continue;
        if (rank == dst) {
            xplan::rowsorted_tables(keys, n, m, order[r], rowoff[r], scratch);
        } else if ((int)r == rank) {
            Layout L;
            const std::vector<uint64_t> no_parts;
            build_layout(n, SketchWords{keys, nullptr, nullptr, 0}, LayoutQuery{1, m.rb, m.re, &no_parts, m.kreq, m.extra.empty() ? nullptr : &m.extra}, L);
            std::vector<std::pair<uint64_t, uint64_t>> wsegs;
            wanted_order(n, m.rb, m.re, &m.extra, wsegs, true);
            for (auto &w : wsegs)
                for (uint64_t s = w.first - m.rb; s < w.second - m.rb; ++s) order[r].push_back(L.perm[s]);
            rowoff[r] = L.rowoff_w;
        }
    }
    const xplan::Schedule S = xplan::schedule(n, modes, nparts, dst, rank, rowoff);
    std::vector<uint64_t> msgs, ents, ro;
    std::vector<uint32_t> ord, md;
    for (size_t q = 0; q < S.M; ++q)
        for (int src = 0; src < S.world; ++src) msgs.push_back(S.msg(q, src).first), msgs.push_back(S.msg(q, src).cnt);
    for (const xplan::Ent &e : S.ents) ents.insert(ents.end(), {(uint64_t)e.src, e.pos0, (uint64_t)e.row0, (uint64_t)e.nrows});
    for (uint32_t r = 0; r < rs.world; ++r) {
        ro.insert(ro.end(), rowoff[r].begin(), rowoff[r].end());
        ord.insert(ord.end(), order[r].begin(), order[r].end());
        md.insert(md.end(), {modes[r].rowsorted ? 1u : 0u, (uint32_t)modes[r].nparts(), modes[r].kreq});
    }
    info[0] = S.stage_total, info[1] = S.ent_off, info[2] = S.tab_bytes;
    void *const none[14] = {};
    if (!bufs) bufs = none;
    bool fits = hand_back(S.total, bufs[0], counts[0]);
    fits = hand_back(msgs, bufs[1], counts[1]) && fits;
    fits = hand_back(S.post, bufs[2], counts[2]) && fits;
    fits = hand_back(S.gate, bufs[3], counts[3]) && fits;
    fits = hand_back(S.part_end, bufs[4], counts[4]) && fits;
    fits = hand_back(S.stage_off, bufs[5], counts[5]) && fits;
    fits = hand_back(S.tab_off, bufs[6], counts[6]) && fits;
    fits = hand_back(ents, bufs[7], counts[7]) && fits;
    fits = hand_back(S.round_ent, bufs[8], counts[8]) && fits;
    fits = hand_back(S.round_rows, bufs[9], counts[9]) && fits;
    fits = hand_back(ro, bufs[10], counts[10]) && fits;
    fits = hand_back(ord, bufs[11], counts[11]) && fits;
    fits = hand_back(md, bufs[12], counts[12]) && fits;
    fits = hand_back(modes[(size_t)rank].cut, bufs[13], counts[13]) && fits;
    return fits ? 0 : -2;
}

}  // extern "C"
