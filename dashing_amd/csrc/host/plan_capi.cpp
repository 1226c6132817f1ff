// plan_capi.cpp -- CPU test hook of the pure-host planner (../plan.cpp): builds a layout and a pair plan for given
// per-sketch keys exactly as engine.hip does and checks the plan against its contract, so the schedule that replaces
// dist_loop / perform_core_op (src/sketch_and_cmp.h:785-880, :699-710) is unit-tested without a GPU
// (tests/test_plan.py).  Also the sequential build of the clusters' union-find (dsh_plan_uf_labels, at the end) and the band rule of
// the greedy representatives (dshh_greedy_bands) and the band walk all five band consumers share (dshh_threshold_bands), and the
// sequential build of the linkage clusters (dsh_plan_linkage_labels, dsh_plan_linkage_loose: ../linkage.h).  Built into
// libdashing_host.so; not part of the GPU C-ABI.
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../linkage.h"
#include "../mst.h"
#include "../plan.h"
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

}  // namespace

// mode: 0 triangle rows [rb, re) (want_sorted decides the layout), 1 rectangle rows [rb,re) x cols [cb,ce) (identity
// layout), 2 sorted_rows (whole sorted layout, rows [rb,re) index plane columns: shards / band-wise kNN), 3 triangle
// rows in ROW-SORTED parts (the wanted rows one key-ordered run, parts = runs of whole tile rows of that order).
// stats out: [0] tiles, [1] bands, [2] items, [3] parts with an event, [4] planes per tile x 100, [5] Npad, [6] P,
// [7] rounds summed over the bands, each in its own round (a round of fragments counted as one), [8] overflow fragments,
// [9] (with round_items given) the round the first band was planned for.
// round_items: the tile kernel's round (256 x the items per workgroup, engine.hip); 0 = the planner's default
// extra: further wanted segments {b0, e0, ...} (plan.h, row sets; modes 0 and 3 with a sorted layout only)
static int plan_check(uint64_t n, const uint32_t *keys, int mode, int want_sorted, uint64_t rb, uint64_t re, uint64_t cb,
                      uint64_t ce, uint32_t nparts, int want_parts, int p, uint64_t cum_budget, int lockstep, int nsplit,
                      int ls_item_chunks, const std::vector<uint64_t> &extra, uint64_t *stats, char *err, size_t cap,
                      uint32_t round_items = 0, const SparseCheck *sc = nullptr)
{
    Err E{err, cap};
    if (re > n) re = n;
    const bool rowsorted = mode == 3;
    if (rowsorted) mode = 0, want_sorted = 1, want_parts = 1;
    if (mode == 1 || !want_sorted) want_sorted = mode == 2 ? 1 : 0;
    if (mode == 2) want_sorted = 1;
    std::vector<uint64_t> parts;
    uint64_t lrb = 0, lre = n;
    if (want_sorted && mode == 0) lrb = rb, lre = re;
    if (want_sorted && !rowsorted) range_parts(n, lrb, lre, std::max<uint32_t>(want_parts ? nparts : 1, 1), parts);
    if (!extra.empty() && !(want_sorted && mode == 0)) return E.fail("extra segments need a sorted triangle layout");
    Layout L;
    build_layout(keys, n, want_sorted, lrb, lre, parts, L, rowsorted ? std::max<uint32_t>(nparts, 1) : 0, extra.empty() ? nullptr : &extra,
                 sc ? sc->gcnt : nullptr, sc ? sc->thr : nullptr, sc ? sc->thr_cap : 0);
    // the wanted segments, main range first
    std::vector<std::pair<uint64_t, uint64_t>> wsegs;  // (the wanted order: extra segments first, then the main range)
    wanted_order(n, lrb, lre, &extra, wsegs, rowsorted);
    auto in_rows = [&](uint64_t i) {
        for (auto &w : wsegs)
            if (i >= w.first && i < w.second) return true;
        return false;
    };
    uint64_t nw = 0, wspan = 0;
    for (auto &w : wsegs) nw += w.second - w.first, wspan += tri_span(n, w.first, w.second);
    if (want_sorted && mode == 0 && L.nwanted != nw) return E.fail("nwanted %llu != %llu", (unsigned long long)L.nwanted, (unsigned long long)nw);
    if (rowsorted) {  // one key-ordered run per wanted segment, cuts on whole tile rows of the wanted order, row offsets of the rank's buffer
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
        if (L.part_w.size() - 1 > std::max<uint32_t>(nparts, 1)) return E.fail("row-sorted: more parts than asked for");
        uint64_t acc = 0, w_ = 0;
        if (L.rowoff_w.size() != nw + 1) return E.fail("row-sorted: rowoff_w size");
        for (auto &w : wsegs)
            for (uint64_t s = w.first - lrb; s < w.second - lrb; ++s, ++w_) {
                if (s >= L.rowoff.size() || L.rowoff[s] != acc || L.rowoff_w[w_] != acc) return E.fail("row-sorted: rowoff[%llu]", (unsigned long long)s);
                acc += n - 1 - L.perm[s];
            }
        if (L.rowoff_w.back() != acc || acc != wspan) return E.fail("row-sorted: the rows do not add up to the span");
    }
    // ---- layout: perm is a permutation of the columns; the parts hold exactly their rows; block stats are right
    const uint64_t col0 = want_sorted ? lrb : 0;
    if (L.ncols != n - col0) return E.fail("ncols %llu != %llu", (unsigned long long)L.ncols, (unsigned long long)(n - col0));
    if (L.Npad % kTile || L.Npad < L.ncols || L.Npad >= L.ncols + kTile) return E.fail("bad Npad %u", L.Npad);
    std::vector<uint8_t> seen(n, 0);
    for (uint64_t s = 0; s < L.ncols; ++s) {
        const uint32_t g = L.perm[s];
        if (g < col0 || g >= n || seen[g]) return E.fail("perm[%llu] = %u is out of range or repeated", (unsigned long long)s, g);
        seen[g] = 1;
    }
    if (want_sorted) {
        uint64_t s = 0;
        for (size_t q = 0; q + 1 < L.parts.size(); ++q)
            for (uint64_t r = L.parts[q]; r < L.parts[q + 1]; ++r, ++s)
                if (L.perm[s] < L.parts[q] || L.perm[s] >= L.parts[q + 1])
                    return E.fail("column %llu holds sketch %u, not a row of part %zu", (unsigned long long)s, L.perm[s], q);
        if (!rowsorted && extra.empty()) {
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
        if (!extra.empty())
            for (uint64_t s2 = 0; s2 < L.ncols; ++s2) {
                // rows to the right of a position are larger unless they share its run: position order = row order between runs
                const uint64_t b = s2 / kTile * kTile;
                if (in_rows(L.perm[s2]) != in_rows(L.perm[b])) return E.fail("block %llu mixes wanted and other rows", (unsigned long long)(b / kTile));
            }
        if (L.whole)
            for (uint64_t i = 0; i < n; ++i)
                if (L.perm[n + L.perm[i]] != i) return E.fail("inverse permutation wrong at %llu", (unsigned long long)i);
    }
    Tuning tu;
    const uint64_t m = 1ull << p;
    tu.W = (uint32_t)std::max<uint64_t>(1, m / 32);
    tu.kc = tu.W >= 32 ? 32 : 16;
    tu.cum_bytes = p <= 15 ? 2 : 4;
    tu.cum_budget = cum_budget;
    tu.nsplit = nsplit;
    tu.lockstep = lockstep && tu.W >= (uint32_t)tu.kc;
    tu.ls_item_chunks = ls_item_chunks;
    if (round_items) tu.round_items = round_items;
    if (round_items > 512) tu.small_round_items = 512;  // (as engine.hip under pair_groups = auto)
    tu.p = p;
    if (sc) tu.sparse_planes = sc->planes, tu.sparse_cap = sc->cap, tu.sparse_sided = sc->sided;
    PairQuery q;
    q.rect = mode == 1;
    q.sorted_rows = mode == 2;
    q.want_parts = want_parts && mode == 0 && want_sorted;
    q.row_begin = rb;
    q.row_end = re;
    q.col_begin = cb;
    q.col_end = ce;
    PairPlan pp;
    const bool any = build_pairs(L, q, tu, pp);
    for (int i = 0; i < 9; ++i) stats[i] = 0;
    stats[5] = L.Npad;
    stats[6] = L.P;
    // ---- every wanted pair is owned by exactly one (tile, lane) -- the `active` predicate of k_finalize
    std::vector<uint8_t> hit;
    uint64_t wanted = 0;
    auto orig = [&](uint64_t s) -> uint64_t { return L.perm[s]; };
    if (mode == 1) {
        const uint64_t nr = re > rb ? re - rb : 0, nc = ce > cb ? ce - cb : 0;
        wanted = nr * nc;
        hit.assign(wanted, 0);
    } else {
        hit.assign(n * n, 0);
        for (uint64_t i = rb; i < re; ++i) wanted += n - 1 - i;
        for (size_t x = 0; x + 1 < extra.size(); x += 2)
            for (uint64_t i = extra[x]; i < extra[x + 1]; ++i) wanted += n - 1 - i;
        if (mode == 2) {
            wanted = 0;
            for (uint64_t si = rb; si < re; ++si) wanted += n - 1 - si;
        }
    }
    if (!any) {
        if (wanted) return E.fail("nothing planned although %llu pairs are wanted", (unsigned long long)wanted);
        return 0;
    }
    const std::vector<U4> &T = pp.T;
    uint64_t got = 0, planes_sum = 0;
    for (const U4 &t : T) {
        if (t.z > t.w || t.w > L.P) return E.fail("tile (%u,%u) has the plane range [%u,%u) of %u", t.x, t.y, t.z, t.w, L.P);
        planes_sum += t.w - t.z;
        for (uint32_t a = 0; a < kTile; ++a)
            for (uint32_t b = 0; b < kTile; ++b) {
                const uint64_t si = (uint64_t)t.x * kTile + a, sj = (uint64_t)t.y * kTile + b;
                if (si >= L.ncols || sj >= L.ncols) continue;
                const uint64_t i = orig(si), j = orig(sj);
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
                    if (active && !extra.empty() && !in_rows(oi))
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
    // ---- bands cover the tiles in order and respect the scratch budget (a single tile may exceed it)
    size_t at = 0;
    if (pp.bands.size() != pp.segs.size() || pp.bands.size() != pp.band_items.size()) return E.fail("band bookkeeping sizes differ");
    std::vector<int> part_done(pp.nparts, 0);
    int last_part = -1;
    for (size_t bi = 0; bi < pp.bands.size(); ++bi) {
        const auto &bd = pp.bands[bi];
        if (bd.first != at || bd.second <= bd.first || bd.second > T.size()) return E.fail("band %zu = [%zu,%zu) does not follow %zu", bi, bd.first, bd.second, at);
        at = bd.second;
        if (bd.second - bd.first > 1 && (bd.second - bd.first) * pp.per_tile_bytes > cum_budget)
            return E.fail("band %zu needs %llu bytes of C(v), budget %llu", bi, (unsigned long long)((bd.second - bd.first) * pp.per_tile_bytes), (unsigned long long)cum_budget);
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
            if (q.want_parts)
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
        std::vector<uint32_t> next(bd.second - bd.first);
        for (size_t t = bd.first; t < bd.second; ++t) next[t - bd.first] = pp.chunks[t].x;
        std::vector<std::vector<std::pair<uint32_t, uint32_t>>> per(bd.second - bd.first);
        const uint32_t cpp_ = tu.W >= (uint32_t)tu.kc ? tu.W / tu.kc : 1;
        // overflow fragments (plan.h): the band's LAST band_frags items, each inside one plane, equal in length, at most one
        // round of them; the whole items in front of them a whole number of rounds
        const uint32_t nfr = bi < pp.band_frags.size() ? pp.band_frags[bi] : 0u;
        const uint32_t bri = bi < pp.band_round.size() ? pp.band_round[bi] : 0u;  // the round this band was planned for
        if (bri != tu.round_items && !(tu.small_round_items && bri == tu.small_round_items)) return E.fail("band %zu: round of %u items", bi, bri);
        if (bi == 0 && round_items) stats[9] = bri;  // (dshh_plan_check_ri only: its callers pass ten slots)
        if (nfr > bi_.second - bi_.first || nfr > bri) return E.fail("band %zu: %u fragments", bi, nfr);
        if (nfr && (!tu.lockstep || (bi_.second - bi_.first - nfr) % bri)) return E.fail("band %zu: fragments behind %zu whole items", bi, bi_.second - bi_.first - nfr);
        stats[8] += nfr;
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
    // ---- sparse outer planes: every plane of a tile's range is in the tile's chunk range (checked above against
    // pp.chunks) or has exactly one sparse item, never both; a routed plane's sets are inside the cap
    // With the sided route every plane of a tile's range is in exactly one route: the dense remainder [pb + below, pe - above)
    // -- one range -- or one sparse item; an item's list block is within its bound, in the item's polarity, for every sketch.
    if (pp.sp.size() != T.size() || pp.spb.size() != T.size() || pp.band_sp_items.size() != pp.bands.size()) return E.fail("sparse bookkeeping sizes differ");
    const bool sided_chk = sc && sc->thr && sc->sided != 0 && pp.sided_items > 0;
    {
        const uint32_t cpp_ = tu.W >= (uint32_t)tu.kc ? tu.W / tu.kc : 1;
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
                        const uint32_t th = sc->thr[orig(sx)];
                        if (la ? v > (int)((th >> 8) & 0xFFu) : v < (int)(th & 0xFFu))
                            return E.fail("sparse item %zu: sketch %llu of the list block is outside its bound at v = %d", k, (unsigned long long)orig(sx), v);
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
                            const uint32_t key = keys[orig(sx)], g = sc->gcnt[orig(sx)];
                            const uint32_t own = v >= key_T(key) ? (g & 0xFFFFu) : v == key_T(key) - 1 ? g >> 16 : 65535u;
                            if (own > tu.sparse_cap) return E.fail("sparse item %zu: sketch %llu may hold %u positions", k, (unsigned long long)orig(sx), own);
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
    }
    for (uint32_t qd = 0; qd < pp.nparts; ++qd)
        if (part_done[qd] != 1) return E.fail("part %u never completes", qd);
    if (pp.nparts) {  // the tile counts the signalling k_finalize waits for
        uint64_t tsum = 0;
        if (pp.part_tiles.size() != pp.nparts) return E.fail("part_tiles has %zu entries for %u parts", pp.part_tiles.size(), pp.nparts);
        for (uint32_t c : pp.part_tiles) tsum += c;
        if (tsum != T.size()) return E.fail("the parts hold %llu tiles of %zu", (unsigned long long)tsum, T.size());
    }
    if (q.want_parts && pp.nparts + 1 != L.part_w.size()) return E.fail("%u parts planned, layout has %zu", pp.nparts, L.part_w.size() - 1);
    // ---- the two device lists describe the same tiles
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
            {  // tile row by tile row inside the segment, columns ascending (the tile rows come in the wanted order: the
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
        }
    stats[0] = T.size();
    stats[1] = pp.bands.size();
    stats[2] = pp.items.size();
    stats[3] = pp.nparts;
    stats[4] = T.empty() ? 0 : planes_sum * 100 / T.size();
    // rounds of the lockstep tile kernel over all bands (a band of k items takes ceil(k / round_items) rounds)
    if (sc) stats[10] = pp.sp_items.size(), stats[11] = pp.slabs.size();
    if (sc && sc->routes6) stats[12] = pp.sided_items, stats[13] = pp.transposed_items, stats[14] = pp.table_slabs;
    stats[7] = 0;
    for (size_t b = 0; b < pp.band_items.size(); ++b) {
        const uint32_t nfr = b < pp.band_frags.size() ? pp.band_frags[b] : 0u;
        const uint32_t bri = pp.band_round[b];
        stats[7] += (pp.band_items[b].second - pp.band_items[b].first - nfr + bri - 1) / bri + (nfr ? 1 : 0);
    }
    return 0;
}

extern "C" {

int dshh_plan_check(uint64_t n, const uint32_t *keys, int mode, int want_sorted, uint64_t rb, uint64_t re, uint64_t cb,
                    uint64_t ce, uint32_t nparts, int want_parts, int p, uint64_t cum_budget, int lockstep, int nsplit,
                    int ls_item_chunks, uint64_t *stats, char *err, size_t cap)
{
    return plan_check(n, keys, mode, want_sorted, rb, re, cb, ce, nparts, want_parts, p, cum_budget, lockstep, nsplit, ls_item_chunks,
                      std::vector<uint64_t>(), stats, err, cap);
}

// the same check with the tile kernel's round given (a multiple of 256: 256 x the items per workgroup)
int dshh_plan_check_ri(uint64_t n, const uint32_t *keys, int mode, int want_sorted, uint64_t rb, uint64_t re, uint64_t cb,
                       uint64_t ce, uint32_t nparts, int want_parts, int p, uint64_t cum_budget, int lockstep, int nsplit,
                       int ls_item_chunks, uint32_t round_items, uint64_t *stats, char *err, size_t cap)
{
    Err E{err, cap};
    if (round_items == 0 || round_items % 256) return E.fail("round_items %u is not a positive multiple of 256", round_items);
    return plan_check(n, keys, mode, want_sorted, rb, re, cb, ce, nparts, want_parts, p, cum_budget, lockstep, nsplit, ls_item_chunks,
                      std::vector<uint64_t>(), stats, err, cap, round_items);
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
    return plan_check(n, keys, mode, want_sorted, rb, re, 0, 0, nparts, want_parts, p, cum_budget, 1, 0, 64, std::vector<uint64_t>(), stats, err,
                      cap, round_items, &sc);
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
    return plan_check(n, keys, mode, want_sorted, rb, re, 0, 0, nparts, want_parts, p, cum_budget, 1, 0, 64, std::vector<uint64_t>(), stats, err,
                      cap, round_items, &sc);
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
    return plan_check(n, keys, rowsorted ? 3 : 0, 1, rb, re, 0, 0, rowsorted ? nparts : 1, 1, p, cum_budget, 1, 0, 64, extra, stats, err, cap);
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
