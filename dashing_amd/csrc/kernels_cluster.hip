// kernels_cluster.hip -- connected components on the device: the clusters at a threshold (cluster.hip).
//
// parent is a uint32 [n] array in device memory, and parent[x] <= x AT ALL TIMES.  Only two kinds of write exist (uf.h):
//   hook              atomicCAS(&parent[r], r, s) with s < r: a root goes under a smaller root
//   path shortening   atomicMin(&parent[x], g) with g an ancestor of x that was read before
// Both keep the invariant: paths strictly decrease, cycles cannot form, and the final root of a component is its smallest
// member -- the label, with no renumbering pass and no dependence on launch geometry or the order atomics arrive in.
// Every access to parent[] inside the uniting kernels is a relaxed agent-scope atomic (the XCDs have separate L2s; a
// plain load could also be served by a CU's L1 for ever).  A stale value would still be the node or one of its ancestors:
// a retry, never a wrong merge -- correctness rests on the atomicity of the hook alone.
// Every loop is bounded: find and the hook's retry loop count their steps against `cap` (the host passes n + 1; a path has
// at most n - 1 links, and the larger root of a hook strictly decreases per retry).  On overrun the thread stores a nonzero
// code into the one-word err buffer and returns; the host reads err once, at the end of the call.  Unreachable while the
// invariant holds.
//   k_cc_init    parent[x] = x
//   k_cc_seed    unite(x, labels_in[x]): an earlier labelling to continue from
//   k_cc_edges   unite(lhs[e], rhs[e]), grid-stride; self loops and repeated edges are legal
//   k_cc_csr     unite(row_begin + r, col[h]) for the hits of a CSR; the row of a hit by binary search in row_ptr
//   k_cc_band    the hot one: a band of dense values walked as thr_walk.h lays down (ThrRows, one wave per 4096-value
//                chunk of a row, one aligned float4 per lane per step, ragged edges value by value, as k_thr_count
//                does); a passing value at column j unites j with the chunk's row.  No count, scan or emit pass, and
//                no hit is written
//   k_cc_labels  a launch of its own, so that all hooks are visible: labels[x] = find(x); roots counted with __ballot +
//                popcount and one atomicAdd per wave
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "thr_walk.h"
#include "uf_dev.h"

namespace dsh {

namespace {

__global__ __launch_bounds__(256) void k_cc_init(uint32_t *__restrict__ parent, uint64_t n)
{
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += (uint64_t)gridDim.x * 256) parent[x] = (uint32_t)x;
}

__global__ __launch_bounds__(256) void k_cc_seed(uint32_t *parent, const uint32_t *__restrict__ labels_in, uint64_t n, uint32_t cap,
                                                 uint32_t *err)
{
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += (uint64_t)gridDim.x * 256) {
        const uint32_t l = labels_in[x];
        if (l < n && l != (uint32_t)x && cc_unite(parent, (uint32_t)x, l, cap, err) == kUfOverrun) return;
    }
}

__global__ __launch_bounds__(256) void k_cc_edges(uint32_t *parent, const uint32_t *__restrict__ lhs, const uint32_t *__restrict__ rhs,
                                                  uint64_t n_edges, uint64_t n, uint32_t cap, uint32_t *err)
{
    for (uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x; e < n_edges; e += (uint64_t)gridDim.x * 256) {
        const uint32_t a = lhs[e], b = rhs[e];
        if (a < n && b < n && a != b && cc_unite(parent, a, b, cap, err) == kUfOverrun) return;  // (the host has checked the range)
    }
}

// hits [h0, h0 + cnt) of a CSR whose row pointer (rows + 1 entries, non-decreasing) is whole on the device; col holds
// the cnt columns of these hits.  The row of hit h is the last r with row_ptr[r] <= h: at most 64 halvings.
__global__ __launch_bounds__(256) void k_cc_csr(uint32_t *parent, const unsigned long long *__restrict__ row_ptr, uint64_t rows,
                                                uint64_t row_begin, const uint32_t *__restrict__ col, uint64_t h0, uint64_t cnt,
                                                uint64_t n, uint32_t cap, uint32_t *err)
{
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < cnt; x += (uint64_t)gridDim.x * 256) {
        const uint64_t h = h0 + x;
        uint64_t lo = 0, hi = rows;  // row_ptr[lo] <= h < row_ptr[hi]
        for (int it = 0; it < 64 && hi - lo > 1; ++it) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (row_ptr[mid] <= h) lo = mid;
            else hi = mid;
        }
        const uint64_t a = row_begin + lo;
        const uint32_t b = col[x];
        if (a < n && b < n && (uint32_t)a != b && cc_unite(parent, (uint32_t)a, b, cap, err) == kUfOverrun) return;
    }
}

// The walk of thr_walk.h, triangle rows only (thr_tri_row: launch_cc_band takes no rectangle).
__global__ __launch_bounds__(256) void k_cc_band(const float *__restrict__ vals, ThrRows g, float t, int descending, uint32_t *parent,
                                                 uint32_t cap, uint32_t *err)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r = blockIdx.x;
    const uint32_t ch = blockIdx.y * 4 + wave;
    if (ch >= g.nchunks) return;
    const uint64_t i = g.row0 + r;
    const ThrRow row = thr_tri_row(g, r);
    uint64_t begin, end;
    if (!thr_chunk(row, ch, begin, end)) return;
    // the row is the same for the whole chunk: its root is kept (every lane its own copy: any member of i's set that was
    // a root when read serves) and refreshed after a hook
    uint32_t root_i = uf_find<UfDevice>(parent, (uint32_t)i, cap);
    if (root_i == kUfOverrun) {
        __hip_atomic_store(err, kUfErrFind, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    for (uint64_t idx = thr_first(begin, lane); idx < end; idx += kThrStep) {
        float v[4];
        const uint32_t m = thr_flags(vals, idx, begin, end, t, descending, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!((m >> c) & 1u)) continue;
            const uint32_t j = row.colbase + (uint32_t)(idx + c - row.rowoff);
            const uint32_t rj = uf_find<UfDevice>(parent, j, cap);
            if (rj == root_i) continue;  // the common case at loose thresholds: nothing to write
            if (rj == kUfOverrun) {
                __hip_atomic_store(err, kUfErrFind, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                return;
            }
            root_i = cc_unite(parent, root_i, rj, cap, err);
            if (root_i == kUfOverrun) return;
        }
    }
}

__global__ __launch_bounds__(256) void k_cc_labels(uint32_t *parent, uint64_t n, uint32_t cap, uint32_t *__restrict__ labels,
                                                   unsigned long long *n_roots, uint32_t *err)
{
    const uint64_t nround = (n + 255) / 256 * 256;  // whole waves take part in the ballot
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < nround; x += (uint64_t)gridDim.x * 256) {
        bool root = false;
        if (x < n) {
            uint32_t l = uf_find<UfDevice>(parent, (uint32_t)x, cap);
            if (l == kUfOverrun) {
                __hip_atomic_store(err, kUfErrFind, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                l = (uint32_t)x;
            }
            labels[x] = l;
            root = l == (uint32_t)x;
        }
        const unsigned long long b = __ballot(root);
        if ((threadIdx.x & 63u) == 0 && b) atomicAdd(n_roots, (unsigned long long)__popcll(b));
    }
}

uint32_t cc_grid(uint64_t items)
{
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 8192);
}

}  // namespace

hipError_t launch_cc_init(hipStream_t st, uint32_t *parent, uint64_t n)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_cc_init, dim3(cc_grid(n)), dim3(256), 0, st, parent, n);
    return hipGetLastError();
}

hipError_t launch_cc_seed(hipStream_t st, uint32_t *parent, const uint32_t *labels_in, uint64_t n, uint32_t cap, uint32_t *err)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_cc_seed, dim3(cc_grid(n)), dim3(256), 0, st, parent, labels_in, n, cap, err);
    return hipGetLastError();
}

hipError_t launch_cc_edges(hipStream_t st, uint32_t *parent, const uint32_t *lhs, const uint32_t *rhs, uint64_t n_edges, uint64_t n,
                           uint32_t cap, uint32_t *err)
{
    if (!n_edges) return hipSuccess;
    hipLaunchKernelGGL(k_cc_edges, dim3(cc_grid(n_edges)), dim3(256), 0, st, parent, lhs, rhs, n_edges, n, cap, err);
    return hipGetLastError();
}

hipError_t launch_cc_csr(hipStream_t st, uint32_t *parent, const uint64_t *row_ptr, uint64_t rows, uint64_t row_begin,
                         const uint32_t *col, uint64_t h0, uint64_t cnt, uint64_t n, uint32_t cap, uint32_t *err)
{
    if (!cnt || !rows) return hipSuccess;
    hipLaunchKernelGGL(k_cc_csr, dim3(cc_grid(cnt)), dim3(256), 0, st, parent, reinterpret_cast<const unsigned long long *>(row_ptr), rows,
                       row_begin, col, h0, cnt, n, cap, err);
    return hipGetLastError();
}

hipError_t launch_cc_band(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *parent, uint32_t cap,
                          uint32_t *err)
{
    if (g.rows == 0 || g.rect) return hipSuccess;
    hipLaunchKernelGGL(k_cc_band, thr_grid(g), dim3(256), 0, st, vals, g, t, descending, parent, cap, err);
    return hipGetLastError();
}

hipError_t launch_cc_labels(hipStream_t st, uint32_t *parent, uint64_t n, uint32_t cap, uint32_t *labels, uint64_t *n_roots, uint32_t *err)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_cc_labels, dim3(cc_grid(n)), dim3(256), 0, st, parent, n, cap, labels, reinterpret_cast<unsigned long long *>(n_roots),
                       err);
    return hipGetLastError();
}

}  // namespace dsh
