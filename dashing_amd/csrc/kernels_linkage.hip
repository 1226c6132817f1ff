// kernels_linkage.hip -- complete- and average-linkage clusters at a threshold on the device (linkage.hip).
// The step logic is linkage.h, the code the CPU tests run sequentially; here it runs with one workgroup per component.
//
// The components of the graph of passing pairs (at least two members each) come from the host as a member CSR: comp[n] the
// component of a slot (kLkNone: a singleton), rank[n] its index inside it, moff / mem the members in slot order, coff the
// first cell of the component's m x m matrix in the scratch of its batch.
//   k_lk_fill_band   a band of dense values walked as thr_walk.h lays down (the geometry of k_cc_band): a value whose row and
//                    column share a component of the batch is stored as a cell at (rank i, rank j) and (rank j, rank i).  A
//                    wave whose row is in no component of the batch returns at once
//   k_lk_fill_pairs  the same store for the values of an explicit pair list (the pairs route: k_gs_enum + pairs_run_chunk)
//   k_linkage<L>     one workgroup of 256 threads per component, which it agglomerates to the end.  Per alive row the best
//                    partner nn / its cell nnv, the sizes, the alive flags and root[] (the cluster a member is in) live in LDS
//                    up to lds_max members and in global scratch above; the matrix stays in global memory as a full square, so
//                    thread k, which owns row k, reads column k: consecutive addresses across the lanes of a wave.  Per step:
//                      1. every thread the best of its rows' candidates (i, nn[i]); a workgroup reduction under lk_better
//                      2. the pass test; the workgroup leaves the loop as one
//                      3. row and column a of the matrix from rows a and b (lk_update_cell), b dies, a holds both sizes
//                      4. nn of every alive row: a full rescan where it was a or b, else one comparison with the new cell
//                         (lk_update_nn); the candidates (a, k) reduce to the rescan of row a
//                    then labels[member] = the slot of its root.
// Bounds: at most m - 1 steps and scans of m cells, both against `cap` (the host passes the largest m + 1); on overrun one
// thread stores a code into the one-word err buffer and the workgroup returns (unreachable in a correct kernel; the CPU build
// of linkage.h reaches it with a small cap).  No workgroup waits for another; no atomics but that store; no inline assembly.
// Every store into the matrices is checked against the scratch's size first.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "linkage.h"
#include "thr_walk.h"

namespace dsh {

namespace {

constexpr uint32_t kLkThreads = 256;

// the cells (i, j) and (j, i) of the pair of slots i != j with the value v, if one component of the batch holds both
template <int L>
__device__ __forceinline__ void lk_store(const LkComps &C, const LkBatch &B, uint32_t ci, uint32_t i, uint32_t j, float v, int descending)
{
    typedef typename LkCell<L>::T T;
    if (C.comp[j] != ci) return;
    const uint64_t m = C.moff[ci + 1] - C.moff[ci], base = C.coff[ci];
    const uint64_t ri = C.rank[i], rj = C.rank[j];
    if (ri >= m || rj >= m || base + m * m > B.ncells) return;  // (the host's tables keep both false)
    T *cells = (T *)B.cells + base;
    const T x = lk_cell<L>(v, descending);
    cells[ri * m + rj] = x;
    cells[rj * m + ri] = x;
}

template <int L>
__global__ __launch_bounds__(256) void k_lk_fill_band(const float *__restrict__ vals, ThrRows g, LkComps C, LkBatch B, int descending)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r = blockIdx.x;
    const uint32_t ch = blockIdx.y * 4 + wave;
    if (ch >= g.nchunks) return;
    const uint32_t i = (uint32_t)(g.row0 + r);
    const uint32_t ci = C.comp[i];
    if (ci == kLkNone || ci < B.c0 || ci >= B.c1) return;
    const ThrRow row = thr_tri_row(g, r);
    uint64_t begin, end;
    if (!thr_chunk(row, ch, begin, end)) return;
    for (uint64_t idx = thr_first(begin, lane); idx < end; idx += kThrStep) {
        if (idx >= begin && idx + 4 <= end) {
            const float4 q = *reinterpret_cast<const float4 *>(vals + idx);
            const float v[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int c = 0; c < 4; ++c) lk_store<L>(C, B, ci, i, row.colbase + (uint32_t)(idx + c - row.rowoff), v[c], descending);
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (idx + c >= begin && idx + c < end)
                    lk_store<L>(C, B, ci, i, row.colbase + (uint32_t)(idx + c - row.rowoff), vals[idx + c], descending);
        }
    }
}

template <int L>
__global__ __launch_bounds__(256) void k_lk_fill_pairs(const uint32_t *__restrict__ lhs, const uint32_t *__restrict__ rhs,
                                                       const float *__restrict__ vals, uint64_t cnt, uint64_t n, LkComps C, LkBatch B,
                                                       int descending)
{
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < cnt; x += (uint64_t)gridDim.x * 256) {
        const uint32_t i = lhs[x], j = rhs[x];
        if (i >= n || j >= n || i == j) continue;  // (the pair path reports a slot out of range itself)
        const uint32_t ci = C.comp[i];
        if (ci == kLkNone || ci < B.c0 || ci >= B.c1) continue;
        lk_store<L>(C, B, ci, i, j, vals[x], descending);
    }
}

// the best of the workgroup's candidates, in every thread.  red: 256 entries of LDS
template <int L>
__device__ __forceinline__ LkCand<L> lk_wg_best(LkCand<L> *red, const LkCand<L> &mine, int descending)
{
    const uint32_t tid = threadIdx.x;
    red[tid] = mine;
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = kLkThreads / 2; s > 0; s >>= 1) {
        if (tid < s && lk_better<L>(red[tid + s], red[tid], descending)) red[tid] = red[tid + s];
        __syncthreads();
    }
    const LkCand<L> best = red[0];
    __syncthreads();  // (red is written again by the next reduction)
    return best;
}

template <int L>
__global__ __launch_bounds__(256) void k_linkage(LkComps C, LkBatch B, LkThr thr, uint32_t lds_max, uint32_t cap, uint32_t *labels,
                                                 uint32_t *err)
{
    typedef typename LkCell<L>::T T;
    typedef LkCand<L> Cand;
    extern __shared__ __attribute__((aligned(16))) char lk_smem[];  // red[256] | nnv | size | nn | root | alive (carves of 16 bytes)
    Cand *red = reinterpret_cast<Cand *>(lk_smem);
    const uint32_t tid = threadIdx.x;
    const uint32_t c = B.c0 + blockIdx.x;
    const uint32_t m0 = C.moff[c], m = C.moff[c + 1] - m0;
    const uint64_t base = C.coff[c];
    if (m > cap || base + (uint64_t)m * m > B.ncells || m0 < B.mbase || (uint64_t)(m0 - B.mbase) + m > B.members) {
        if (tid == 0) __hip_atomic_store(err, kLkErrScan, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    T *cells = (T *)B.cells + base;
    T *nnv;
    uint32_t *size, *nn, *root, *alive;
    if (m <= lds_max) {
        const uint32_t mp = (m + 3u) & ~3u;
        char *p = lk_smem + kLkThreads * sizeof(Cand);
        nnv = reinterpret_cast<T *>(p), p += (size_t)mp * sizeof(T);
        size = reinterpret_cast<uint32_t *>(p), p += (size_t)mp * 4;
        nn = reinterpret_cast<uint32_t *>(p), p += (size_t)mp * 4;
        root = reinterpret_cast<uint32_t *>(p), p += (size_t)mp * 4;
        alive = reinterpret_cast<uint32_t *>(p);
    } else {  // nnv[members] | size[members] | nn | root | alive of the batch, this component's part
        const uint64_t s0 = m0 - B.mbase, M = B.members;
        nnv = (T *)B.state + s0;
        uint32_t *w = reinterpret_cast<uint32_t *>((T *)B.state + M);
        size = w + s0, nn = w + M + s0, root = w + 2 * M + s0, alive = w + 3 * M + s0;
    }
    const int desc = thr.descending;
    for (uint32_t i = tid; i < m; i += kLkThreads) alive[i] = 1, size[i] = 1, root[i] = i;
    __syncthreads();
    for (uint32_t i = tid; i < m; i += kLkThreads) lk_set_nn<L>(lk_scan_row<L>(cells, m, i, alive, size, desc), i, nn, nnv);
    __syncthreads();
#pragma unroll 1
    for (uint32_t step = 0;; ++step) {
        Cand mine = lk_none<L>();
        for (uint32_t i = tid; i < m; i += kLkThreads) {
            if (!alive[i]) continue;
            const Cand x = lk_row_cand<L>(i, size, nn, nnv);
            if (lk_better<L>(x, mine, desc)) mine = x;
        }
        const Cand best = lk_wg_best<L>(red, mine, desc);
        if (best.a == kLkNone || !lk_pass<L>(best, thr)) break;
        if (step >= cap) {
            if (tid == 0) __hip_atomic_store(err, kLkErrStep, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        const uint32_t a = best.a, b = best.b;
        if (a >= m || b >= m || a >= b) {  // (a candidate is built from indices below m)
            if (tid == 0) __hip_atomic_store(err, kLkErrScan, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
        for (uint32_t k = tid; k < m; k += kLkThreads)
            if (alive[k] && k != a && k != b) lk_update_cell<L>(cells, m, a, b, k);
        __syncthreads();
        if (tid == 0) {
            alive[b] = 0;
            size[a] += size[b];
        }
        __syncthreads();
        Cand rowa = lk_none<L>();
        for (uint32_t k = tid; k < m; k += kLkThreads) {
            if (root[k] == b) root[k] = a;
            if (!alive[k] || k == a) continue;
            const Cand x = lk_update_nn<L>(cells, m, a, b, k, alive, size, nn, nnv, desc);
            if (lk_better<L>(x, rowa, desc)) rowa = x;
        }
        const Cand ra = lk_wg_best<L>(red, rowa, desc);
        if (tid == 0) lk_set_nn<L>(ra, a, nn, nnv);
        __syncthreads();
    }
    __syncthreads();
    for (uint32_t i = tid; i < m; i += kLkThreads) {
        const uint32_t r = root[i];
        if (r < m) labels[C.mem[m0 + i]] = C.mem[m0 + r];
    }
}

uint32_t lk_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 8192); }

}  // namespace

size_t linkage_lds_bytes(int linkage, uint32_t m)
{
    const size_t mp = ((size_t)m + 3) & ~(size_t)3;
    return kLkThreads * sizeof(LkCand<kLkAverage>) + mp * ((linkage == kLkAverage ? 8 : 4) + 16);
}

hipError_t launch_lk_fill_band(hipStream_t st, int linkage, const float *vals, const ThrRows &g, const LkComps &C, const LkBatch &B, int descending)
{
    if (g.rows == 0) return hipSuccess;
    if (g.rect) return hipErrorInvalidValue;
    if (linkage == kLkSingle) hipLaunchKernelGGL(k_lk_fill_band<kLkSingle>, thr_grid(g), dim3(256), 0, st, vals, g, C, B, descending);
    else if (linkage == kLkComplete) hipLaunchKernelGGL(k_lk_fill_band<kLkComplete>, thr_grid(g), dim3(256), 0, st, vals, g, C, B, descending);
    else hipLaunchKernelGGL(k_lk_fill_band<kLkAverage>, thr_grid(g), dim3(256), 0, st, vals, g, C, B, descending);
    return hipGetLastError();
}

hipError_t launch_lk_fill_pairs(hipStream_t st, int linkage, const uint32_t *lhs, const uint32_t *rhs, const float *vals, uint64_t cnt,
                                uint64_t n, const LkComps &C, const LkBatch &B, int descending)
{
    if (!cnt) return hipSuccess;
    const dim3 grid(lk_grid(cnt));
    if (linkage == kLkSingle) hipLaunchKernelGGL(k_lk_fill_pairs<kLkSingle>, grid, dim3(256), 0, st, lhs, rhs, vals, cnt, n, C, B, descending);
    else if (linkage == kLkComplete) hipLaunchKernelGGL(k_lk_fill_pairs<kLkComplete>, grid, dim3(256), 0, st, lhs, rhs, vals, cnt, n, C, B, descending);
    else hipLaunchKernelGGL(k_lk_fill_pairs<kLkAverage>, grid, dim3(256), 0, st, lhs, rhs, vals, cnt, n, C, B, descending);
    return hipGetLastError();
}

template <int L>
static hipError_t launch_lk(hipStream_t st, const LkComps &C, const LkBatch &B, const LkThr &thr, uint32_t lds_max, size_t lds, uint32_t cap,
                            uint32_t *labels, uint32_t *err)
{
    const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(k_linkage<L>), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_linkage<L>, dim3(B.c1 - B.c0), dim3(kLkThreads), lds, st, C, B, thr, lds_max, cap, labels, err);
    return hipGetLastError();
}

hipError_t launch_linkage(hipStream_t st, int linkage, const LkComps &C, const LkBatch &B, float threshold, int descending, uint32_t lds_max,
                          uint32_t lds_members, uint32_t cap, uint32_t *labels, uint32_t *err)
{
    if (B.c1 <= B.c0) return hipSuccess;
    const LkThr thr = lk_threshold(threshold, descending);
    const size_t lds = linkage_lds_bytes(linkage, std::min(lds_members, lds_max));
    if (linkage == kLkSingle) return launch_lk<kLkSingle>(st, C, B, thr, lds_max, lds, cap, labels, err);
    if (linkage == kLkComplete) return launch_lk<kLkComplete>(st, C, B, thr, lds_max, lds, cap, labels, err);
    return launch_lk<kLkAverage>(st, C, B, thr, lds_max, lds, cap, labels, err);
}

}  // namespace dsh
