// kernels_threshold.hip -- device-side selection of the values that pass a threshold, as CSR (threshold.hip).
//
// The input is what the compare path left in a band buffer, walked as thr_walk.h lays down: rows of the packed triangle or
// of a rectangle, a row cut into chunks of kThrChunk values; a chunk belongs to ONE wave, which walks it front to back, so
// the order inside a row is the column order by construction:
//   k_thr_count  hits per chunk                                   cnt[r * NC + ch]
//   k_thr_scan   exclusive scan of cnt over all chunks, row-major  off[...] (absolute: the hits of earlier bands included),
//                the band's piece of row_ptr and the running total
//   k_thr_emit   the same walk again; a hit goes to off[chunk] + its rank inside the chunk.  The rank of a lane's hit
//                comes from the 64-bit __ballot masks of the step and the population count of the lanes below it:
//                no sort, and no atomic cursor whose order of arrival would show in the output.
// Offsets of values and of hits are 64-bit throughout.  Nothing is written at or beyond `cap`.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "thr_walk.h"

namespace dsh {

namespace {

__global__ __launch_bounds__(256) void k_thr_count(const float *__restrict__ vals, ThrRows g, float t, int descending,
                                                   uint32_t *__restrict__ cnt)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r = blockIdx.x;
    const uint32_t ch = blockIdx.y * 4 + wave;
    if (ch >= g.nchunks) return;
    uint64_t begin, end;
    uint32_t mine = 0;
    if (thr_chunk(thr_row(g, r), ch, begin, end)) {
        float v[4];
        for (uint64_t idx = thr_first(begin, lane); idx < end; idx += kThrStep)
            mine += __popc(thr_flags(vals, idx, begin, end, t, descending, v));
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (lane == 0) cnt[r * g.nchunks + ch] = mine;
}

// One workgroup: off[e] = *total + sum of cnt[0 .. e), off[m] and *total = the new total, row_ptr[r] = off[r * nchunks].
__global__ __launch_bounds__(1024) void k_thr_scan(const uint32_t *__restrict__ cnt, uint64_t m, uint32_t nchunks,
                                                   unsigned long long *__restrict__ off, unsigned long long *__restrict__ row_ptr,
                                                   unsigned long long *__restrict__ total)
{
    __shared__ uint32_t wsum[16];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned long long carry = *total;
    __syncthreads();  // every thread has read the total before thread 0 rewrites it
    for (uint64_t base = 0; base < m; base += 4096) {
        const uint64_t e0 = base + 4 * (uint64_t)tid;
        uint32_t c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = e0 + q < m ? cnt[e0 + q] : 0u;
        const uint32_t s = c[0] + c[1] + c[2] + c[3];  // (a tile holds at most 4096 * kThrChunk hits: 2^24)
        uint32_t incl = s;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_up(incl, d, 64);
            if (lane >= (uint32_t)d) incl += o;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, tile = 0;
#pragma unroll
        for (uint32_t w = 0; w < 16; ++w) {
            const uint32_t x = wsum[w];
            before += w < wave ? x : 0u;
            tile += x;
        }
        __syncthreads();  // wsum is rewritten by the next tile
        unsigned long long o = carry + before + (incl - s);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (e0 + q < m) {
                off[e0 + q] = o;
                if ((e0 + q) % nchunks == 0) row_ptr[(e0 + q) / nchunks] = o;
            }
            o += c[q];
        }
        carry += tile;
    }
    if (tid == 0) {
        off[m] = carry;
        *total = carry;
    }
}

__global__ __launch_bounds__(256) void k_thr_emit(const float *__restrict__ vals, ThrRows g, float t, int descending,
                                                  const unsigned long long *__restrict__ off, uint64_t sub, uint64_t cap,
                                                  uint32_t *__restrict__ col, float *__restrict__ val)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r = blockIdx.x;
    const uint32_t ch = blockIdx.y * 4 + wave;
    if (ch >= g.nchunks) return;
    const uint64_t e = r * g.nchunks + ch;
    uint64_t pos = off[e];  // wave-uniform
    if (off[e + 1] == pos) return;  // (also every chunk beyond the row's end)
    pos -= sub;
    const ThrRow row = thr_row(g, r);
    uint64_t begin, end;
    (void)thr_chunk(row, ch, begin, end);  // (not behind the row's end: the chunk has hits)
    for (uint64_t sb = thr_first(begin, 0); sb < end; sb += kThrStep) {  // wave-uniform trip count: every lane takes part in the ballots
        const uint64_t idx = sb + 4 * lane;
        float v[4];
        const uint32_t m = idx < end ? thr_flags(vals, idx, begin, end, t, descending, v) : 0u;
        uint32_t below = 0, all = 0;  // hits of the lanes below this one / of the whole step
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned long long b = __ballot((m >> c) & 1u);
            below += __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            all += __popcll(b);
        }
        uint64_t p = pos + below;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if ((m >> c) & 1u) {
                if (p < cap) {
                    col[p] = row.colbase + (uint32_t)(idx + c - row.rowoff);
                    val[p] = v[c];
                }
                ++p;
            }
        }
        pos += all;
    }
}

}  // namespace

hipError_t launch_thr_count(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *cnt)
{
    if (g.rows == 0) return hipSuccess;
    hipLaunchKernelGGL(k_thr_count, thr_grid(g), dim3(256), 0, st, vals, g, t, descending, cnt);
    return hipGetLastError();
}

hipError_t launch_thr_scan(hipStream_t st, const uint32_t *cnt, uint64_t m, uint32_t nchunks, uint64_t *off, uint64_t *row_ptr,
                           uint64_t *total)
{
    hipLaunchKernelGGL(k_thr_scan, dim3(1), dim3(1024), 0, st, cnt, m, nchunks, reinterpret_cast<unsigned long long *>(off),
                       reinterpret_cast<unsigned long long *>(row_ptr), reinterpret_cast<unsigned long long *>(total));
    return hipGetLastError();
}

hipError_t launch_thr_emit(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, const uint64_t *off,
                           uint64_t sub, uint64_t cap, uint32_t *col, float *val)
{
    if (g.rows == 0 || cap == 0) return hipSuccess;
    hipLaunchKernelGGL(k_thr_emit, thr_grid(g), dim3(256), 0, st, vals, g, t, descending,
                       reinterpret_cast<const unsigned long long *>(off), sub, cap, col, val);
    return hipGetLastError();
}

}  // namespace dsh
