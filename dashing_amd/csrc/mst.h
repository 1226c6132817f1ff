// mst.h -- the step logic of the minimum spanning tree of the pair values (kernels_mst.hip on the device, host/plan_capi.cpp
// for the CPU tests; DESIGN.md 4.16, include/dashing_hip.h has the contract).  One source for both, in the idiom of uf.h and
// linkage.h: the words, the offers, the two picks and the emit test are __host__ __device__ and reach memory through a policy
//   A::load64(p)       the value at p
//   A::max64(p, val)   p = max(p, val)          A::max32 likewise
//   A::min64(p, val)   p = min(p, val)
// (relaxed agent-scope atomics on the device, plain accesses in the sequential host build); mst_run_seq at the end is the
// sequential driver of the host build, and mst.hip runs the same steps as kernels, one launch per step.
//
// Borůvka rounds.  labels[x] is the root of x's component when the round starts (uf.h: its smallest member).  Per round:
//   offers   every edge of G (a value that is not NaN and passes the cutoff) whose ends lie in different components offers
//            itself to both ends: best_v[x] = the largest (key << 32 | ~partner), 0 = none.  The key is lk_key (vkey.h's
//            value_key32 for both sides of the build: larger = better, never 0 for a value), so the word of a real value is
//            never 0, and on equal values the smaller partner wins -- which is the better edge in the total order whichever
//            side of x the partner lies on.
//   pick 1   ckey[c] = the best key among the members of component c
//   pick 2   cedge[c] = the smallest (i << 32 | j), i < j, among the members' offers that hold that key: the component's
//            best outgoing edge in the total order (better value, then smaller i, then smaller j)
//   emit     c emits its edge unless the component at the other end chose the same edge and has the smaller label: a mutual
//            choice is emitted once.  The order is strict and total, so the chosen edges close no cycle.
// A round that emits nothing ends the run.  The components with an outgoing edge at least halve per round: at most
// floor(log2 n) + 1 rounds emit, kMstMaxRounds bounds the loop, and an overrun is an error, not a spin.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "linkage.h"
#include "uf.h"

#if defined(__HIPCC__)
#define DSH_MST_FN __host__ __device__ __forceinline__
#else
#define DSH_MST_FN inline
#endif

namespace dsh {

constexpr uint32_t kMstMaxRounds = 34;
constexpr uint64_t kMstNoEdge = ~0ull;
constexpr uint32_t kMstErrRounds = 3;  // beside kUfErrFind, kUfErrHook
constexpr uint32_t kMstErrRoom = 4;    // more than n - 1 edges: unreachable, kept from writing behind the buffer

// the float predicate of dsh_dist_threshold (thr_walk.h: thr_pass) for both sides of the build; NaN on either side: false
DSH_MST_FN bool mst_pass(float v, float cutoff, int descending) { return descending ? v >= cutoff : v <= cutoff; }

DSH_MST_FN uint64_t mst_word(uint32_t key, uint32_t partner) { return (uint64_t)key << 32 | (uint32_t)~partner; }
DSH_MST_FN uint32_t mst_word_key(uint64_t w) { return (uint32_t)(w >> 32); }
DSH_MST_FN uint32_t mst_word_partner(uint64_t w) { return ~(uint32_t)w; }

// the value a key stands for (+0.0 for either zero): value_of_key32 of vkey.h for both sides of the build
DSH_MST_FN float mst_value(uint32_t u, int descending)
{
    if (!descending) u = ~u;
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    float v;
    __builtin_memcpy(&v, &u, sizeof v);
    return v;
}

// an offer to x.  best_v only grows within a round, so a stale read costs one redundant max and never loses an update
template <class A>
DSH_MST_FN void mst_offer(uint64_t *best_v, uint32_t x, uint64_t w)
{
    if (A::load64(best_v + x) < w) A::max64(best_v + x, w);
}

template <class A>
DSH_MST_FN void mst_pick_key(const uint64_t *best_v, const uint32_t *labels, uint32_t *ckey, uint32_t x)
{
    const uint64_t w = best_v[x];
    if (w) A::max32(ckey + labels[x], mst_word_key(w));
}

template <class A>
DSH_MST_FN void mst_pick_edge(const uint64_t *best_v, const uint32_t *labels, const uint32_t *ckey, uint64_t *cedge, uint32_t x)
{
    const uint64_t w = best_v[x];
    if (!w || mst_word_key(w) != ckey[labels[x]]) return;
    const uint32_t y = mst_word_partner(w);
    A::min64(cedge + labels[x], x < y ? (uint64_t)x << 32 | y : (uint64_t)y << 32 | x);
}

// does x, if it is the root of a component with an outgoing edge, emit that edge (i, j)?
DSH_MST_FN bool mst_emits(const uint32_t *labels, const uint32_t *ckey, const uint64_t *cedge, uint32_t x, uint32_t &i, uint32_t &j)
{
    if (labels[x] != x || !ckey[x]) return false;
    const uint64_t e = cedge[x];
    if (e == kMstNoEdge) return false;  // (never with a key: the member that holds it has offered its edge)
    i = (uint32_t)(e >> 32), j = (uint32_t)e;
    const uint32_t other = labels[i] == x ? labels[j] : labels[i];
    return !(other < x && ckey[other] == ckey[x] && cedge[other] == e);
}

struct MstEdge {
    uint32_t key, i, j;
};
// the total order: the better value, then the smaller i, then the smaller j
inline bool mst_before(const MstEdge &a, const MstEdge &b) { return a.key != b.key ? a.key > b.key : a.i != b.i ? a.i < b.i : a.j < b.j; }

// the edges a run left in arbitrary order, as the caller gets them
inline void mst_sorted_out(std::vector<MstEdge> &e, int descending, uint32_t *lhs, uint32_t *rhs, float *val)
{
    std::sort(e.begin(), e.end(), mst_before);
    for (size_t x = 0; x < e.size(); ++x) lhs[x] = e[x].i, rhs[x] = e[x].j, val[x] = mst_value(e[x].key, descending);
}

struct MstPlain : UfPlain {
    static DSH_MST_FN uint64_t load64(const uint64_t *p) { return *p; }
    static DSH_MST_FN void max64(uint64_t *p, uint64_t v) { if (v > *p) *p = v; }
    static DSH_MST_FN void max32(uint32_t *p, uint32_t v) { if (v > *p) *p = v; }
    static DSH_MST_FN void min64(uint64_t *p, uint64_t v) { if (v < *p) *p = v; }
};

// The sequential driver over a host triangle (dsh_tri_index order): the forest's edges in arbitrary order into `out`, the
// final roots into parent (labels[x] = uf_find).  Returns 0, or the give-up code; *rounds = the rounds that emitted.
inline uint32_t mst_run_seq(uint64_t n, const float *tri, int descending, float cutoff, uint32_t round_cap, std::vector<uint32_t> &parent,
                            std::vector<MstEdge> &out, uint32_t *rounds)
{
    const uint32_t cap = (uint32_t)std::min<uint64_t>(n + 1, 0xFFFFFFFFull);
    std::vector<uint32_t> labels(n), ckey(n);
    std::vector<uint64_t> best_v(n), cedge(n);
    parent.resize(n);
    for (uint64_t x = 0; x < n; ++x) parent[x] = (uint32_t)x;
    out.clear();
    *rounds = 0;
    for (;;) {
        for (uint64_t x = 0; x < n; ++x) {
            if ((labels[x] = uf_find<UfPlain>(parent.data(), (uint32_t)x, cap)) == kUfOverrun) return kUfErrFind;
            best_v[x] = 0, ckey[x] = 0, cedge[x] = kMstNoEdge;
        }
        uint64_t idx = 0;
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = i + 1; j < n; ++j, ++idx) {
                const float v = tri[idx];
                if (!mst_pass(v, cutoff, descending) || labels[i] == labels[j]) continue;
                const uint32_t key = lk_key(v, descending);
                mst_offer<MstPlain>(best_v.data(), i, mst_word(key, j));
                mst_offer<MstPlain>(best_v.data(), j, mst_word(key, i));
            }
        for (uint32_t x = 0; x < n; ++x) mst_pick_key<MstPlain>(best_v.data(), labels.data(), ckey.data(), x);
        for (uint32_t x = 0; x < n; ++x) mst_pick_edge<MstPlain>(best_v.data(), labels.data(), ckey.data(), cedge.data(), x);
        const size_t before = out.size();
        for (uint32_t x = 0; x < n; ++x) {
            uint32_t i, j, why = 0;
            if (!mst_emits(labels.data(), ckey.data(), cedge.data(), x, i, j)) continue;
            if (out.size() + 1 >= n) return kMstErrRoom;
            out.push_back(MstEdge{ckey[x], i, j});
            if (uf_unite<UfPlain>(parent.data(), i, j, cap, &why) == kUfOverrun) return why;
        }
        if (out.size() == before) return 0;
        if (++*rounds > round_cap) return kMstErrRounds;
        if (out.size() + 1 == n) return 0;  // a spanning tree: nothing is left to offer
    }
}

// The sorted edge list as a merge table in scipy's convention: leaves 0 .. n - 1, step s joins the current clusters of
// lhs[s] and rhs[s] into cluster n + s; za[s] < zb[s] the two ids, zv[s] = val[s], zsize[s] the members.  False: an edge names
// a node >= n or joins two nodes that are already united (the list is not a forest), or an id would not fit 32 bits.
inline bool mst_linkage(uint64_t n, const uint32_t *lhs, const uint32_t *rhs, const float *val, uint64_t n_edges, uint32_t *za, uint32_t *zb,
                        float *zv, uint32_t *zsize)
{
    if (n_edges >= std::max<uint64_t>(n, 1) || n + n_edges > 0xFFFFFFFFull) return false;
    const uint32_t cap = (uint32_t)(n + 1);
    std::vector<uint32_t> parent(n), id(n), size(n, 1);
    for (uint64_t x = 0; x < n; ++x) parent[x] = id[x] = (uint32_t)x;
    for (uint64_t s = 0; s < n_edges; ++s) {
        if (lhs[s] >= n || rhs[s] >= n) return false;
        const uint32_t a = uf_find<UfPlain>(parent.data(), lhs[s], cap), b = uf_find<UfPlain>(parent.data(), rhs[s], cap);
        if (a == b || a == kUfOverrun || b == kUfOverrun) return false;
        const uint32_t lo = std::min(a, b), hi = std::max(a, b);
        za[s] = std::min(id[a], id[b]), zb[s] = std::max(id[a], id[b]);
        zv[s] = val[s];
        zsize[s] = size[lo] += size[hi];
        parent[hi] = lo;  // the hook of uf.h: the larger root under the smaller
        id[lo] = (uint32_t)(n + s);
    }
    return true;
}

}  // namespace dsh
