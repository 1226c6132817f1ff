// kernels_group.hip -- per-group statistics and medoids of a labelling (group_stats.hip).
//
// Per slot x three accumulators in device memory, all integers, so that the result depends on no band size, route, launch
// geometry or order of arrival of atomics:
//   cnt[x]   uint32 add   included pairs (x, y), y in x's group (included: v not NaN and |v| < 2)
//   sum[x]   64-bit add   sum of q(v) = llrint(v * 2^30) over them (|q| < 2^31, at most 2^32 - 2 terms: inside int64)
//   wkey[x]  uint32 max   ~value_key32(v) (vkey.h) of the WORST included value: 0 = none, a larger key is a worse value
// The number of atomics does not grow with the number of matching pairs:
//   k_gs_rows    a band of dense values walked as thr_walk.h lays down (ThrRows, one wave per 4096-value chunk of a row, one
//                aligned float4 per lane per step, ragged edges value by value).  A lane loads the labels of its four columns
//                next to the values and accumulates row i's (cnt, sum, wkey) over the columns with labels[i]; the wave
//                reduces across lanes; at most ONE set of atomics per wave, none for a chunk without a matching column
//   k_gs_cols    the band's contribution to its COLUMNS: a thread owns column j and walks the rows i < j of one slab of
//                kGsSlab band rows (consecutive threads read consecutive addresses of a row; the slab's labels in LDS; a
//                value is loaded only where the labels match), accumulates privately: at most one set per (column, slab)
//   k_gs_enum    pairs route: the intra-group pairs [x0, x0 + cnt) of the member CSR as lhs = the larger slot, rhs = the
//                smaller; the pair index to (group, a, b) through the prefix of pair counts by bounded binary search
//   k_gs_pairs   pairs route: a chunk's values folded into both ends; a wave whose pairs share the lhs (the enumeration
//                order makes that the rule) reduces that side first
//   k_gs_medoid  three launches over the slots with the key (largest cnt, best sum, smallest slot), each an integer atomic
//                per group (index = the label) over the members that equal the one before: free of ties by construction
//   k_gs_finish  medoid[x] gathered from x's group, worst decoded, cnt and sum copied; a NULL output is not written
// Every loop is bounded; no thread waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "thr_walk.h"
#include "vkey.h"

namespace dsh {

namespace {

constexpr uint32_t kGsSlab = 512;  // band rows a thread of k_gs_cols walks

struct GsAcc {
    uint32_t c = 0, w = 0;
    long long s = 0;
    __device__ __forceinline__ void fold(float v, int descending)
    {
        if (!(fabsf(v) < 2.0f)) return;  // NaN, and what no measure of real sketches gives
        ++c;
        s += __double2ll_rn((double)v * 1073741824.0);  // exact product, round to nearest even
        w = max(w, ~value_key32(v, descending));
    }
    // afterwards lane 0 holds the wave's totals
    __device__ __forceinline__ void wave_reduce()
    {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            c += __shfl_xor(c, m, 64);
            s += __shfl_xor(s, m, 64);
            w = max(w, __shfl_xor(w, m, 64));
        }
    }
    __device__ __forceinline__ void commit(uint32_t x, uint32_t *cnt, unsigned long long *sum, uint32_t *wkey) const
    {
        if (!c) return;
        (void)atomicAdd(cnt + x, c);
        (void)atomicAdd(sum + x, (unsigned long long)s);
        (void)atomicMax(wkey + x, w);
    }
};

// The walk of thr_walk.h, triangle rows only (thr_tri_row: launch_gs_rows takes no rectangle).
__global__ __launch_bounds__(256) void k_gs_rows(const float *__restrict__ vals, ThrRows g, const uint32_t *__restrict__ labels,
                                                 int descending, uint32_t *cnt, unsigned long long *sum, uint32_t *wkey)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r = blockIdx.x;
    const uint32_t ch = blockIdx.y * 4 + wave;
    if (ch >= g.nchunks) return;
    const uint64_t i = g.row0 + r;
    const ThrRow row = thr_tri_row(g, r);
    uint64_t begin, end;
    if (!thr_chunk(row, ch, begin, end)) return;
    const uint32_t li = labels[i];
    GsAcc a;
    for (uint64_t idx = thr_first(begin, lane); idx < end; idx += kThrStep) {
        // the load of thr_flags (thr_walk.h) with the label test in the place of thr_pass, written out: as a predicate handed to a
        // shared load the kernel came out with other register counts (36 -> 31 VGPRs, 28 -> 34 SGPRs)
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        uint32_t m = 0;
        if (idx >= begin && idx + 4 <= end) {
            const float4 q = *reinterpret_cast<const float4 *>(vals + idx);
            v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
            const uint32_t j = row.colbase + (uint32_t)(idx - row.rowoff);
#pragma unroll
            for (int c = 0; c < 4; ++c) m |= (labels[j + c] == li ? 1u : 0u) << c;
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (idx + c >= begin && idx + c < end) {
                    v[c] = vals[idx + c];
                    m |= (labels[row.colbase + (uint32_t)(idx + c - row.rowoff)] == li ? 1u : 0u) << c;
                }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if ((m >> c) & 1u) a.fold(v[c], descending);
    }
    a.wave_reduce();
    if (lane == 0) a.commit((uint32_t)i, cnt, sum, wkey);
}

// block (x, y): the slab y of band rows [y kGsSlab, ...) and the 256 columns from the slab's first row + 1 + 256 x on
__global__ __launch_bounds__(256) void k_gs_cols(const float *__restrict__ vals, ThrRows g, const uint32_t *__restrict__ labels,
                                                 int descending, uint32_t *cnt, unsigned long long *sum, uint32_t *wkey)
{
    __shared__ uint32_t lab[kGsSlab];
    const uint64_t r0 = (uint64_t)blockIdx.y * kGsSlab;
    if (r0 >= g.rows) return;
    const uint64_t r1 = r0 + kGsSlab < g.rows ? r0 + kGsSlab : g.rows;
    const uint64_t i0 = g.row0 + r0;
    const uint64_t jb = i0 + 1 + (uint64_t)blockIdx.x * 256;
    if (jb >= g.n) return;  // (the whole block: before the barrier)
    for (uint32_t t = threadIdx.x; t < (uint32_t)(r1 - r0); t += 256) lab[t] = labels[i0 + t];
    __syncthreads();
    const uint64_t j = jb + threadIdx.x;
    if (j >= g.n) return;
    const uint32_t lj = labels[j];
    const uint64_t first = g.n - 1 - g.row0;
    uint64_t off = band_rowoff(first, r0);  // start of band row r0, then of each next one
    const uint64_t rend = j - g.row0 < r1 ? j - g.row0 : r1;  // rows i < j only
    GsAcc a;
    for (uint64_t r = r0; r < rend; ++r) {  // at most kGsSlab steps
        if (lab[r - r0] == lj) a.fold(vals[off + (j - (g.row0 + r) - 1)], descending);
        off += first - r;
    }
    a.commit((uint32_t)j, cnt, sum, wkey);
}

// ppre[ng + 1]: pairs before each group of at least two members (strictly increasing), moff[ng + 1]: where its members start
// in mem (ascending slots inside a group).  Pair t of a group of s members is (a, b), b < a < s, t = a (a - 1) / 2 + b.
__global__ __launch_bounds__(256) void k_gs_enum(const unsigned long long *__restrict__ ppre, const uint32_t *__restrict__ moff,
                                                 const uint32_t *__restrict__ mem, uint64_t ng, uint64_t x0, uint64_t cnt,
                                                 uint32_t *__restrict__ lhs, uint32_t *__restrict__ rhs)
{
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < cnt; x += (uint64_t)gridDim.x * 256) {
        const uint64_t h = x0 + x;
        uint64_t lo = 0, hi = ng;  // ppre[lo] <= h < ppre[hi]
        for (int it = 0; it < 64 && hi - lo > 1; ++it) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (ppre[mid] <= h) lo = mid;
            else hi = mid;
        }
        const uint64_t t = h - ppre[lo];
        const uint64_t s = (uint64_t)moff[lo + 1] - moff[lo];
        uint64_t a = (uint64_t)((1.0 + sqrt(1.0 + 8.0 * (double)t)) * 0.5);
        a = a < 1 ? 1 : (a > s - 1 ? s - 1 : a);
        for (int it = 0; it < 4 && a * (a - 1) / 2 > t; ++it) --a;       // (the square root errs by less than one)
        for (int it = 0; it < 4 && (a + 1) * a / 2 <= t; ++it) ++a;
        const uint64_t b = t - a * (a - 1) / 2;
        const uint32_t *mm = mem + moff[lo];
        lhs[x] = mm[a < s ? a : s - 1];
        rhs[x] = mm[b < s ? b : 0];
    }
}

__global__ __launch_bounds__(256) void k_gs_pairs(const uint32_t *__restrict__ lhs, const uint32_t *__restrict__ rhs,
                                                  const float *__restrict__ vals, uint64_t n_pairs, uint64_t n, int descending,
                                                  uint32_t *cnt, unsigned long long *sum, uint32_t *wkey)
{
    const uint64_t nround = (n_pairs + 255) / 256 * 256;  // whole waves take part in the reduction
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < nround; x += (uint64_t)gridDim.x * 256) {
        uint32_t a = 0xFFFFFFFFu, b = 0;
        GsAcc acc;
        if (x < n_pairs) {
            a = lhs[x], b = rhs[x];
            if (a < n && b < n) acc.fold(vals[x], descending);  // (the values' own kernels report a slot out of range)
        }
        acc.commit(b, cnt, sum, wkey);
        const uint32_t a0 = __shfl(a, 0, 64);
        if (__all(x >= n_pairs || a == a0)) {  // (x ascends with the lane: lane 0 is the first to be real)
            acc.wave_reduce();
            if ((threadIdx.x & 63u) == 0) acc.commit(a0, cnt, sum, wkey);
        } else {
            acc.commit(a, cnt, sum, wkey);
        }
    }
}

// larger key = better sum
__device__ __forceinline__ unsigned long long sum_key(unsigned long long s, int descending)
{
    const unsigned long long u = s ^ 0x8000000000000000ull;
    return descending ? u : ~u;
}

// step 0: g_cnt[l] = max cnt; 1: g_sum[l] = max sum key among those; 2: g_slot[l] = min slot among those
__global__ __launch_bounds__(256) void k_gs_medoid(int step, const uint32_t *__restrict__ labels, uint64_t n, int descending,
                                                   const uint32_t *__restrict__ cnt, const unsigned long long *__restrict__ sum,
                                                   uint32_t *g_cnt, unsigned long long *g_sum, uint32_t *g_slot)
{
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += (uint64_t)gridDim.x * 256) {
        const uint32_t l = labels[x];
        if (l >= n) continue;  // (the host has checked the range)
        const uint32_t c = cnt[x];
        if (step == 0) {
            if (__hip_atomic_load(g_cnt + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < c) (void)atomicMax(g_cnt + l, c);
            continue;
        }
        if (c != g_cnt[l]) continue;  // (final: written by the launch before)
        const unsigned long long k = sum_key(sum[x], descending);
        if (step == 1) {
            if (__hip_atomic_load(g_sum + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < k) (void)atomicMax(g_sum + l, k);
        } else if (k == g_sum[l]) {
            if (__hip_atomic_load(g_slot + l, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (uint32_t)x) (void)atomicMin(g_slot + l, (uint32_t)x);
        }
    }
}

__global__ __launch_bounds__(256) void k_gs_finish(const uint32_t *__restrict__ labels, uint64_t n, int descending,
                                                   const uint32_t *__restrict__ cnt, const unsigned long long *__restrict__ sum,
                                                   const uint32_t *__restrict__ wkey, const uint32_t *__restrict__ g_slot,
                                                   uint32_t *__restrict__ medoid_out, uint32_t *__restrict__ cnt_out,
                                                   long long *__restrict__ sum_out, float *__restrict__ worst_out)
{
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < n; x += (uint64_t)gridDim.x * 256) {
        const uint32_t l = labels[x];
        if (medoid_out) medoid_out[x] = l < n ? g_slot[l] : (uint32_t)x;
        if (cnt_out) cnt_out[x] = cnt[x];
        if (sum_out) sum_out[x] = (long long)sum[x];
        if (worst_out) worst_out[x] = cnt[x] ? value_of_key32(~wkey[x], descending) : __uint_as_float(0x7FC00000u);
    }
}

uint32_t gs_grid(uint64_t items)
{
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((items + 255) / 256, 1), 8192);
}

}  // namespace

hipError_t launch_gs_rows(hipStream_t st, const float *vals, const ThrRows &g, const uint32_t *labels, int descending, const GsAccum &a)
{
    if (g.rows == 0 || g.rect) return hipSuccess;
    hipLaunchKernelGGL(k_gs_rows, thr_grid(g), dim3(256), 0, st, vals, g, labels, descending, a.cnt,
                       reinterpret_cast<unsigned long long *>(a.sum), a.wkey);
    return hipGetLastError();
}

hipError_t launch_gs_cols(hipStream_t st, const float *vals, const ThrRows &g, const uint32_t *labels, int descending, const GsAccum &a)
{
    if (g.rows == 0 || g.rect || g.n < 2 || g.row0 + 1 >= g.n) return hipSuccess;
    const uint64_t colblocks = (g.n - 1 - g.row0 + 255) / 256, slabs = (g.rows + kGsSlab - 1) / kGsSlab;
    if (slabs > 65535) return hipErrorInvalidValue;  // (a band holds at most 2^20 rows: 2048 slabs)
    hipLaunchKernelGGL(k_gs_cols, dim3((uint32_t)colblocks, (uint32_t)slabs), dim3(256), 0, st, vals, g, labels, descending, a.cnt,
                       reinterpret_cast<unsigned long long *>(a.sum), a.wkey);
    return hipGetLastError();
}

hipError_t launch_gs_enum(hipStream_t st, const uint64_t *ppre, const uint32_t *moff, const uint32_t *mem, uint64_t ngroups, uint64_t x0,
                          uint64_t cnt, uint32_t *lhs, uint32_t *rhs)
{
    if (!cnt || !ngroups) return hipSuccess;
    hipLaunchKernelGGL(k_gs_enum, dim3(gs_grid(cnt)), dim3(256), 0, st, reinterpret_cast<const unsigned long long *>(ppre), moff, mem,
                       ngroups, x0, cnt, lhs, rhs);
    return hipGetLastError();
}

hipError_t launch_gs_pairs(hipStream_t st, const uint32_t *lhs, const uint32_t *rhs, const float *vals, uint64_t n_pairs, uint64_t n,
                           int descending, const GsAccum &a)
{
    if (!n_pairs) return hipSuccess;
    hipLaunchKernelGGL(k_gs_pairs, dim3(gs_grid(n_pairs)), dim3(256), 0, st, lhs, rhs, vals, n_pairs, n, descending, a.cnt,
                       reinterpret_cast<unsigned long long *>(a.sum), a.wkey);
    return hipGetLastError();
}

hipError_t launch_gs_finish(hipStream_t st, const uint32_t *labels, uint64_t n, int descending, const GsAccum &a, uint32_t *g_cnt,
                            uint64_t *g_sum, uint32_t *g_slot, uint32_t *medoid_out, uint32_t *cnt_out, int64_t *sum_out, float *worst_out)
{
    if (!n) return hipSuccess;
    const unsigned long long *sum = reinterpret_cast<const unsigned long long *>(a.sum);
    if (medoid_out)
        for (int step = 0; step < 3; ++step)  // (a launch each: the maxima of one step are final before the next reads them)
            hipLaunchKernelGGL(k_gs_medoid, dim3(gs_grid(n)), dim3(256), 0, st, step, labels, n, descending, a.cnt, sum, g_cnt,
                               reinterpret_cast<unsigned long long *>(g_sum), g_slot);
    hipLaunchKernelGGL(k_gs_finish, dim3(gs_grid(n)), dim3(256), 0, st, labels, n, descending, a.cnt, sum, a.wkey, g_slot, medoid_out,
                       cnt_out, reinterpret_cast<long long *>(sum_out), worst_out);
    return hipGetLastError();
}

}  // namespace dsh
