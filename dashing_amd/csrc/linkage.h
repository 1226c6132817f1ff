// linkage.h -- the step logic of the complete- and average-linkage clusters at a threshold (kernels_linkage.hip on the
// device, host/plan_capi.cpp for the CPU tests; DESIGN.md 4.15, include/dashing_hip.h has the contract).  One source for
// both, in the idiom of uf.h: the cells, the update rule, the exact order of two cluster pairs and the pass test are
// __host__ __device__; lk_run_seq at the end is the sequential driver of the host build, and k_linkage runs the same steps
// with one workgroup per component.
//
// A component of m members holds an m x m symmetric matrix of cells, cell (i, j) at cells[i * m + j]; the index of a member
// is its rank in slot order and a merge always goes into the smaller index, so index order is label order.
//   SINGLE, COMPLETE   a cell is the uint32 key of the best / worst member value (lk_key: larger = better, 0 = blocked)
//   AVERAGE            a cell is the int64 sum S of q(v) over the member pairs (kLkBlocked = blocked); the value of a pair of
//                      clusters is the rational S / c, c = the product of the two sizes, compared by cross-multiplication
//                      in 128-bit integers
// The Lance-Williams updates are exact: the larger / smaller of two keys, S(A u B, C) = S(A, C) + S(B, C), blocked absorbing
// for COMPLETE and AVERAGE.  |q| < 2^31 and c <= 2^32 (the callers refuse AVERAGE components above kLkAvgMaxMembers), so S
// stays inside int64.
//
// Per alive row i, nn[i] is the best partner among all alive others (ties to the smaller index, kLkNone: every partner is
// blocked) and nnv[i] its cell.  The best pair of the step is the best of the rows' candidates (i, nn[i]) under lk_better,
// whose tie rule -- the lexicographically smaller (min, max) -- is for the candidates of one row "the smaller partner".
// Every loop is bounded: a component takes at most m - 1 steps, a scan m cells; both count against `cap` (the callers pass
// m + 1).  An overrun gives kLkErrStep / kLkErrScan: unreachable in a correct build, reached on the CPU with a small cap.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DSH_LK_FN __host__ __device__ __forceinline__
#else
#define DSH_LK_FN inline
#endif

namespace dsh {

constexpr int kLkSingle = 0, kLkComplete = 1, kLkAverage = 2;  // DSH_LINKAGE_*
constexpr uint32_t kLkNone = 0xFFFFFFFFu;
constexpr int64_t kLkBlocked = -0x7FFFFFFFFFFFFFFFll - 1;
constexpr uint32_t kLkErrStep = 1, kLkErrScan = 2;  // what the callers store into their error word
constexpr uint32_t kLkAvgMaxMembers = 65536;         // AVERAGE: c <= 2^32 keeps |S| < 2^63

// value_key32 of vkey.h for both sides of the build, 0 for NaN: larger key = better value, -0.0 = +0.0
DSH_LK_FN uint32_t lk_key(float v, int descending)
{
    if (v != v) return 0u;
    uint32_t u;
    __builtin_memcpy(&u, &v, sizeof u);
    if (u == 0x80000000u) u = 0u;
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return descending ? u : ~u;
}

// q(v) of dsh_group_stats: the product is exact in double, the rounding to nearest even
DSH_LK_FN int64_t lk_q(float v) { return (int64_t)llrint((double)v * 1073741824.0); }

struct LkThr {
    uint32_t key;  // SINGLE, COMPLETE: lk_key(t)
    int64_t Q;     // AVERAGE: q(t)
    int descending;
};

template <int L>
struct LkCell {
    typedef uint32_t T;
};
template <>
struct LkCell<kLkAverage> {
    typedef int64_t T;
};

// the cell of two single slots with the value v
template <int L>
DSH_LK_FN typename LkCell<L>::T lk_cell(float v, int descending)
{
    if constexpr (L == kLkAverage) {
        if (v != v || !(fabsf(v) < 2.f)) return kLkBlocked;  // the rule dsh_group_stats includes a pair by
        return lk_q(v);
    } else {
        return lk_key(v, descending);
    }
}

template <int L>
DSH_LK_FN bool lk_blocked(typename LkCell<L>::T c)
{
    if constexpr (L == kLkAverage) return c == kLkBlocked;
    else return c == 0u;
}

// cell (A u B, C) from the cells (A, C) and (B, C).  SINGLE: 0 is "no value yet", the identity of max
template <int L>
DSH_LK_FN typename LkCell<L>::T lk_merge(typename LkCell<L>::T x, typename LkCell<L>::T y)
{
    if constexpr (L == kLkSingle) return x > y ? x : y;
    else if constexpr (L == kLkComplete) return x < y ? x : y;
    else return (x == kLkBlocked || y == kLkBlocked) ? kLkBlocked : x + y;
}

// a pair of clusters a < b with an unblocked cell; a == kLkNone: no pair
template <int L>
struct LkCand {
    typename LkCell<L>::T v;
    uint32_t a, b;
    uint64_t c;  // the product of the two sizes
};

template <int L>
DSH_LK_FN LkCand<L> lk_none()
{
    LkCand<L> x;
    x.v = 0, x.a = kLkNone, x.b = kLkNone, x.c = 1;
    return x;
}

template <int L>
DSH_LK_FN LkCand<L> lk_cand(uint32_t i, uint32_t j, typename LkCell<L>::T v, uint32_t size_i, uint32_t size_j)
{
    LkCand<L> x;
    x.v = v, x.a = i < j ? i : j, x.b = i < j ? j : i, x.c = (uint64_t)size_i * size_j;
    return x;
}

// x comes strictly before y: the better value, then the lexicographically smaller (a, b).  A total order of distinct pairs.
template <int L>
DSH_LK_FN bool lk_better(const LkCand<L> &x, const LkCand<L> &y, int descending)
{
    if (x.a == kLkNone) return false;
    if (y.a == kLkNone) return true;
    if constexpr (L == kLkAverage) {
        const __int128 l = (__int128)x.v * (__int128)y.c, r = (__int128)y.v * (__int128)x.c;  // x.v / x.c against y.v / y.c
        if (l != r) return descending ? l > r : l < r;
    } else {
        if (x.v != y.v) return x.v > y.v;
    }
    return x.a != y.a ? x.a < y.a : x.b < y.b;
}

template <int L>
DSH_LK_FN bool lk_pass(const LkCand<L> &x, const LkThr &t)
{
    if constexpr (L == kLkAverage) {
        const __int128 s = (__int128)x.v, qc = (__int128)t.Q * (__int128)x.c;
        return t.descending ? s >= qc : s <= qc;
    } else {
        return x.v >= t.key;  // thr_pass in key order: at least as good as t
    }
}

// the best partner of row i among the alive others: column i of the matrix, which symmetry makes row i (on the device the
// lanes of a wave scan neighbouring rows, so they read consecutive addresses)
template <int L>
DSH_LK_FN LkCand<L> lk_scan_row(const typename LkCell<L>::T *cells, uint32_t m, uint32_t i, const uint32_t *alive, const uint32_t *size,
                                int descending)
{
    LkCand<L> best = lk_none<L>();
    const uint32_t si = size[i];
    // (the cell is loaded before it is known to count -- every (j, i) is inside the matrix -- so that the loads of several
    // iterations can be in flight at once: a rescan is one thread's walk over m cells, and its latency is the step's)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 8
#endif
    for (uint32_t j = 0; j < m; ++j) {
        const typename LkCell<L>::T v = cells[(uint64_t)j * m + i];
        if (j == i || !alive[j] || lk_blocked<L>(v)) continue;
        const LkCand<L> x = lk_cand<L>(i, j, v, si, size[j]);
        if (lk_better<L>(x, best, descending)) best = x;
    }
    return best;
}

template <int L>
DSH_LK_FN void lk_set_nn(const LkCand<L> &x, uint32_t i, uint32_t *nn, typename LkCell<L>::T *nnv)
{
    nn[i] = x.a == kLkNone ? kLkNone : (x.a == i ? x.b : x.a);
    nnv[i] = x.v;
}

// the candidate of row i
template <int L>
DSH_LK_FN LkCand<L> lk_row_cand(uint32_t i, const uint32_t *size, const uint32_t *nn, const typename LkCell<L>::T *nnv)
{
    const uint32_t j = nn[i];
    return j == kLkNone ? lk_none<L>() : lk_cand<L>(i, j, nnv[i], size[i], size[j]);
}

// b was merged into a (a < b): the cells of row and column a against an alive k outside the pair
template <int L>
DSH_LK_FN void lk_update_cell(typename LkCell<L>::T *cells, uint32_t m, uint32_t a, uint32_t b, uint32_t k)
{
    const typename LkCell<L>::T v = lk_merge<L>(cells[(uint64_t)a * m + k], cells[(uint64_t)b * m + k]);
    cells[(uint64_t)a * m + k] = v;
    cells[(uint64_t)k * m + a] = v;
}

// ... and, once alive[b] = 0 and size[a] holds both, the nearest neighbour of that k: a full rescan where it was one of the
// two, else one comparison with the new cell.  Returns the candidate (a, k) for the rescan of row a.
template <int L>
DSH_LK_FN LkCand<L> lk_update_nn(const typename LkCell<L>::T *cells, uint32_t m, uint32_t a, uint32_t b, uint32_t k, const uint32_t *alive,
                                 const uint32_t *size, uint32_t *nn, typename LkCell<L>::T *nnv, int descending)
{
    const typename LkCell<L>::T v = cells[(uint64_t)a * m + k];
    const LkCand<L> fresh = lk_blocked<L>(v) ? lk_none<L>() : lk_cand<L>(k, a, v, size[k], size[a]);
    if (nn[k] == a || nn[k] == b) lk_set_nn<L>(lk_scan_row<L>(cells, m, k, alive, size, descending), k, nn, nnv);
    else if (lk_better<L>(fresh, lk_row_cand<L>(k, size, nn, nnv), descending)) lk_set_nn<L>(fresh, k, nn, nnv);
    return fresh;
}

// the threshold of the call
inline LkThr lk_threshold(float t, int descending)
{
    LkThr x;
    x.key = lk_key(t, descending);
    x.Q = (t == t && fabsf(t) < 2.f) ? lk_q(t) : 0;
    x.descending = descending;
    return x;
}

// AVERAGE judges quantised values: the float threshold whose graph of passing pairs is the graph of q(v) against Q = q(t) --
// for a distance the largest float32 with q <= Q, for a similarity the smallest with q >= Q (|t| < 2).  q is monotone and
// q(t) = Q, so the answer lies at the rounding boundary (Q +- 1/2) / 2^30, which is exact in double; the float next to it is
// then moved by single steps (a few at most: the bound of 8 is never reached)
inline float lk_loose_threshold(float t, int descending)
{
    const int64_t Q = lk_q(t);
    const float worse = descending ? -INFINITY : INFINITY;
    float f = (float)(((double)Q + (descending ? -0.5 : 0.5)) / 1073741824.0);
    for (int it = 0; it < 8 && (descending ? lk_q(f) < Q : lk_q(f) > Q); ++it) f = nextafterf(f, -worse);
    for (int it = 0; it < 8; ++it) {
        const float g = nextafterf(f, worse);
        if (descending ? lk_q(g) < Q : lk_q(g) > Q) break;
        f = g;
    }
    return f;
}

// The sequential driver: the m members of ONE component (cells filled by the caller) agglomerated to the end; root[i] = the
// index of the cluster member i ends in.  Returns 0, or the give-up code.
template <int L>
inline uint32_t lk_run_seq(uint32_t m, typename LkCell<L>::T *cells, uint32_t *alive, uint32_t *size, uint32_t *nn,
                           typename LkCell<L>::T *nnv, uint32_t *root, const LkThr &thr, uint32_t cap, uint32_t scan_cap)
{
    if (m > scan_cap) return kLkErrScan;
    const int desc = thr.descending;
    for (uint32_t i = 0; i < m; ++i) alive[i] = 1, size[i] = 1, root[i] = i;
    for (uint32_t i = 0; i < m; ++i) lk_set_nn<L>(lk_scan_row<L>(cells, m, i, alive, size, desc), i, nn, nnv);
    for (uint32_t step = 0;; ++step) {
        LkCand<L> best = lk_none<L>();
        for (uint32_t i = 0; i < m; ++i) {
            if (!alive[i]) continue;
            const LkCand<L> x = lk_row_cand<L>(i, size, nn, nnv);
            if (lk_better<L>(x, best, desc)) best = x;
        }
        if (best.a == kLkNone || !lk_pass<L>(best, thr)) return 0;
        if (step >= cap) return kLkErrStep;
        const uint32_t a = best.a, b = best.b;
        for (uint32_t k = 0; k < m; ++k)
            if (alive[k] && k != a && k != b) lk_update_cell<L>(cells, m, a, b, k);
        alive[b] = 0;
        size[a] += size[b];
        LkCand<L> rowa = lk_none<L>();
        for (uint32_t k = 0; k < m; ++k) {
            if (root[k] == b) root[k] = a;
            if (!alive[k] || k == a) continue;
            const LkCand<L> x = lk_update_nn<L>(cells, m, a, b, k, alive, size, nn, nnv, desc);
            if (lk_better<L>(x, rowa, desc)) rowa = x;
        }
        lk_set_nn<L>(rowa, a, nn, nnv);
    }
}

}  // namespace dsh
