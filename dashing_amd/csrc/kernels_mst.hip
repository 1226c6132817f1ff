// kernels_mst.hip -- the Borůvka rounds of the minimum spanning tree of the pair values (mst.hip, mst.h).
// Per round, each kernel a launch of its own so that what the previous one wrote is visible:
//   k_cc_labels  (kernels_cluster.hip) labels[x] = find(x): the components the round starts with
//   k_mst_band   the hot one: a band of dense values walked as k_cc_band walks it (thr_walk.h: ThrRows, one wave per
//                4096-value chunk of a row, one aligned float4 per lane per step through thr_flags with the cutoff).  A passing
//                value at column j of row i with labels[i] != labels[j] offers (key << 32 | ~j) to best_v[i] and
//                (key << 32 | ~i) to best_v[j] (mst.h).  The columns of a chunk are contiguous, so the lanes' reads of
//                labels[j ..] and best_v[j ..] are coalesced beside the float4 of values.  Row side: the lanes keep their best
//                word in a register, the wave reduces it and issues at most ONE atomicMax per chunk.  Column side: best_v[j] is
//                read first and the atomicMax issued only for a better word; best_v only grows within a round, so a stale read
//                costs a redundant atomic and never loses an update, and after the first rows of a band the atomics are rare.
//                labels[] is constant during the launch (plain loads); best_v is read with relaxed agent-scope atomic loads and
//                written with atomicMax only, as kernels_cluster.hip treats parent[].  Nothing else is written.
//   k_mst_pick_key / k_mst_pick_edge   per component root the best key of its members, then the smallest (i << 32 | j) among
//                the members that hold it
//   k_mst_emit   the roots that emit (mst.h: mst_emits) append their edge -- one atomicAdd per wave, the lanes' places from the
//                ballot -- and unite its ends (uf.h).  The order of the appended edges is arbitrary; the host sorts them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "mst.h"
#include "thr_walk.h"

namespace dsh {

namespace {

struct MstDevice {
    static __device__ __forceinline__ uint32_t load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ uint32_t cas(uint32_t *p, uint32_t cmp, uint32_t val) { return atomicCAS(p, cmp, val); }
    static __device__ __forceinline__ void min(uint32_t *p, uint32_t val) { (void)atomicMin(p, val); }
    static __device__ __forceinline__ uint64_t load64(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ void max64(uint64_t *p, uint64_t v) { (void)atomicMax((unsigned long long *)p, (unsigned long long)v); }
    static __device__ __forceinline__ void max32(uint32_t *p, uint32_t v) { (void)atomicMax(p, v); }
    static __device__ __forceinline__ void min64(uint64_t *p, uint64_t v) { (void)atomicMin((unsigned long long *)p, (unsigned long long)v); }
};

// The walk of thr_walk.h, triangle rows only (thr_tri_row: launch_mst_band takes no rectangle).
__global__ __launch_bounds__(256) void k_mst_band(const float *__restrict__ vals, ThrRows g, float cutoff, int descending,
                                                  const uint32_t *__restrict__ labels, uint64_t *best_v)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r = blockIdx.x;
    const uint32_t ch = blockIdx.y * 4 + wave;
    if (ch >= g.nchunks) return;  // (the whole wave)
    const uint32_t i = (uint32_t)(g.row0 + r);
    const ThrRow row = thr_tri_row(g, r);
    uint64_t begin, end;
    if (!thr_chunk(row, ch, begin, end)) return;
    const uint32_t li = labels[i];
    uint64_t mine = 0;  // the lane's best word for row i
    for (uint64_t idx = thr_first(begin, lane); idx < end; idx += kThrStep) {
        float v[4];
        const uint32_t m = thr_flags(vals, idx, begin, end, cutoff, descending, v);
        if (!m) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!((m >> c) & 1u)) continue;  // (a flag is only set inside [begin, end): j is a column of the row, j < n)
            const uint32_t j = row.colbase + (uint32_t)(idx + c - row.rowoff);
            if (labels[j] == li) continue;  // the common case after the first rounds: nothing to read or write
            const uint32_t key = lk_key(v[c], descending);
            const uint64_t w = mst_word(key, j);
            mine = w > mine ? w : mine;
            mst_offer<MstDevice>(best_v, j, mst_word(key, i));
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)mine, s);
        mine = o > mine ? o : mine;
    }
    if (lane == 0 && mine) mst_offer<MstDevice>(best_v, i, mine);
}

__global__ __launch_bounds__(256) void k_mst_pick_key(const uint64_t *__restrict__ best_v, const uint32_t *__restrict__ labels, uint32_t *ckey,
                                                      uint64_t n)
{
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += (uint64_t)gridDim.x * 256)
        mst_pick_key<MstDevice>(best_v, labels, ckey, (uint32_t)x);
}

__global__ __launch_bounds__(256) void k_mst_pick_edge(const uint64_t *__restrict__ best_v, const uint32_t *__restrict__ labels,
                                                       const uint32_t *__restrict__ ckey, uint64_t *cedge, uint64_t n)
{
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += (uint64_t)gridDim.x * 256)
        mst_pick_edge<MstDevice>(best_v, labels, ckey, cedge, (uint32_t)x);
}

__global__ __launch_bounds__(256) void k_mst_emit(const uint32_t *__restrict__ labels, const uint32_t *__restrict__ ckey,
                                                  const uint64_t *__restrict__ cedge, uint64_t n, uint32_t *parent, uint32_t cap,
                                                  uint32_t *err, MstEdges e)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nround = (n + 255) / 256 * 256;  // whole waves take part in the ballot
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < nround; x += (uint64_t)gridDim.x * 256) {
        uint32_t i = 0, j = 0;
        const bool emits = x < n && mst_emits(labels, ckey, cedge, (uint32_t)x, i, j);
        const unsigned long long b = __ballot(emits);
        if (!b) continue;
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(e.count, (unsigned long long)__popcll(b));
        base = __shfl(base, 0);
        if (!emits) continue;
        const uint64_t at = base + __popcll(b & ((1ull << lane) - 1));
        if (at >= e.room) {  // unreachable: a forest of n nodes has at most n - 1 edges
            __hip_atomic_store(err, kMstErrRoom, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            continue;
        }
        e.lhs[at] = i, e.rhs[at] = j, e.key[at] = ckey[x];
        uint32_t why = 0;
        if (uf_unite<MstDevice>(parent, i, j, cap, &why) == kUfOverrun) __hip_atomic_store(err, why, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

uint32_t mst_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 8192); }

}  // namespace

hipError_t launch_mst_band(hipStream_t st, const float *vals, const ThrRows &g, float cutoff, int descending, const uint32_t *labels,
                           uint64_t *best_v)
{
    if (g.rows == 0 || g.rect) return hipSuccess;
    hipLaunchKernelGGL(k_mst_band, thr_grid(g), dim3(256), 0, st, vals, g, cutoff, descending, labels, best_v);
    return hipGetLastError();
}

hipError_t launch_mst_pick(hipStream_t st, const uint64_t *best_v, const uint32_t *labels, uint32_t *ckey, uint64_t *cedge, uint64_t n)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_mst_pick_key, dim3(mst_grid(n)), dim3(256), 0, st, best_v, labels, ckey, n);
    hipLaunchKernelGGL(k_mst_pick_edge, dim3(mst_grid(n)), dim3(256), 0, st, best_v, labels, ckey, cedge, n);
    return hipGetLastError();
}

hipError_t launch_mst_emit(hipStream_t st, const uint32_t *labels, const uint32_t *ckey, const uint64_t *cedge, uint64_t n, uint32_t *parent,
                           uint32_t cap, uint32_t *err, const MstEdges &e)
{
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_mst_emit, dim3(mst_grid(n)), dim3(256), 0, st, labels, ckey, cedge, n, parent, cap, err, e);
    return hipGetLastError();
}

}  // namespace dsh
