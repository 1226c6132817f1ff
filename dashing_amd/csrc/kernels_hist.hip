// kernels_hist.hip -- the distribution of a band's dense values over caller-given bin edges (hist.hip).
//
// The input is a band buffer walked as thr_walk.h lays down (rows of the packed triangle or of a rectangle, a row cut into
// chunks of kThrChunk values, one wave per chunk, one aligned float4 per lane per step, ragged ends value by value).  Unlike
// the other consumers a workgroup carries state in LDS -- the edges and planes x (n_edges + 2) 32-bit counters, sized from
// n_edges at the launch -- so the grid is BOUNDED (plan::hist_grid) and its waves stride over the band's (row, chunk) units:
// the counters are zeroed once and flushed once per launch, the non-zero ones only, with 64-bit atomic adds into the call's
// uint64 array.  All counting is in integers: the result depends on no band size, grid or order of arrival.
//
//   class(v)    the number of edges that pass v as a threshold would (similarity: e <= v, distance: e < v): a binary search
//               over the edges in LDS, at most kHistSearchSteps steps; NaN is class n_edges + 1.  A lane first tries the class
//               it found last against that class's two edges, kept in registers: in a real collection almost every value
//               falls into one class, and then no search runs at all.
//   counting    one LDS atomic per value on one address would serialise 64-way.  A wave therefore peels classes: the first
//               live lane's counter index is broadcast, the lanes that hold the same index are found with one ballot and
//               counted with ONE add of the population count.  After kHistPeel rounds what is left (a spread over many
//               classes, where the addresses differ anyway) goes lane by lane.  Two rounds, measured: a round costs about as
//               much as the per-lane add it may save, and four rounds were half again as slow at 101 edges (profiles/hist1).
//   overflow    a workgroup's waves take at most kHistMaxIters units of at most kThrChunk values each between zeroing and
//               flush: 4 x (2^18 - 1) x 4096 < 2^32, so no 32-bit counter wraps whatever threshold_band_bytes makes of a
//               band.  plan::hist_grid raises the grid where a band has more units; launch_hist refuses any other grid.
// Every loop is bounded; no thread waits for another beyond the two workgroup barriers.
#include <hip/hip_runtime.h>

#include "../../include/dashing_hip.h"
#include "kernels.h"
#include "plan.h"
#include "thr_walk.h"

namespace dsh {

namespace {

constexpr int kHistSearchSteps = 13;  // candidates 0 .. n_edges <= 4096: 4097 of them, halved 13 times
constexpr int kHistPeel = 2;          // classes a wave counts with one add each before it goes lane by lane
static_assert((1u << (kHistSearchSteps - 1)) >= DSH_HIST_MAX_EDGES, "the search must reach every class");

__device__ __forceinline__ bool hist_passes(float e, float v, int descending) { return descending ? e <= v : e < v; }

// the class a lane found last and the two edges around it
struct HistClass {
    uint32_t k = 0xFFFFFFFFu;
    float lo = 0.f, hi = 0.f;  // edges[k - 1] (k > 0), edges[k] (k < n_edges)
};

__device__ __forceinline__ uint32_t hist_class(const float *edges, uint32_t n_edges, float v, int descending, HistClass &last)
{
    if (v != v) return n_edges + 1;
    if (last.k <= n_edges && (last.k == 0 || hist_passes(last.lo, v, descending)) &&
        (last.k == n_edges || !hist_passes(last.hi, v, descending)))
        return last.k;
    uint32_t lo = 0, hi = n_edges;  // the class lies in [lo, hi]: edges below lo pass, edges from hi on do not
    for (int it = 0; it < kHistSearchSteps && lo < hi; ++it) {
        const uint32_t mid = (lo + hi) >> 1;
        if (hist_passes(edges[mid], v, descending)) lo = mid + 1;
        else hi = mid;
    }
    last.k = lo;
    last.lo = lo > 0 ? edges[lo - 1] : 0.f;
    last.hi = lo < n_edges ? edges[lo] : 0.f;
    return lo;
}

// every lane of the wave calls this (live: the lane holds a value for counter x)
__device__ __forceinline__ void hist_count(uint32_t *cnt, uint32_t x, bool live, uint32_t lane)
{
    unsigned long long rem = __ballot(live);
    for (int round = 0; round < kHistPeel && rem; ++round) {  // (rem is wave-uniform)
        const uint32_t leader = (uint32_t)__ffsll((long long)rem) - 1u;
        const uint32_t x0 = (uint32_t)__shfl((int)x, (int)leader, 64);
        const bool same = live && x == x0;
        const unsigned long long m = __ballot(same);
        if (lane == leader) (void)atomicAdd(cnt + x0, (uint32_t)__popcll(m));
        if (same) live = false;
        rem &= ~m;
    }
    if (live) (void)atomicAdd(cnt + x, 1u);
}

// LDS: float edges[n_edges] | uint32 cnt[planes * (n_edges + 2)], planes = labels ? 2 : 1
__global__ __launch_bounds__(256) void k_hist(const float *__restrict__ vals, ThrRows g, const float *__restrict__ d_edges, uint32_t n_edges,
                                              const uint32_t *__restrict__ labels, int descending, uint64_t units,
                                              unsigned long long *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t hist_lds[];
    float *edges = reinterpret_cast<float *>(hist_lds);
    uint32_t *cnt = hist_lds + n_edges;
    const uint32_t nclass = n_edges + 2, ncnt = labels ? 2 * nclass : nclass;
    for (uint32_t t = threadIdx.x; t < n_edges; t += 256) edges[t] = d_edges[t];
    for (uint32_t t = threadIdx.x; t < ncnt; t += 256) cnt[t] = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    HistClass last;
    // unit u = chunk u % nchunks of band row u / nchunks; at most kHistMaxIters trips (launch_hist)
    for (uint64_t u = (uint64_t)blockIdx.x * 4 + wave; u < units; u += (uint64_t)gridDim.x * 4) {
        const uint64_t r = u / g.nchunks;
        const uint32_t ch = (uint32_t)(u - r * g.nchunks);
        const ThrRow row = thr_row(g, r);
        uint64_t begin, end;
        if (!thr_chunk(row, ch, begin, end)) continue;  // (wave-uniform)
        const uint32_t li = labels ? labels[g.row0 + r] : 0u;
        for (uint64_t sb = thr_first(begin, 0); sb < end; sb += kThrStep) {  // wave-uniform trip count: every lane takes part in the ballots
            const uint64_t idx = sb + 4 * lane;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            uint32_t in = 0, inter = 0;  // bit c: value c lies in the chunk / its column carries another label than the row
            if (idx >= begin && idx + 4 <= end) {
                const float4 q = *reinterpret_cast<const float4 *>(vals + idx);
                v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
                in = 15u;
                if (labels) {
                    const uint32_t j = row.colbase + (uint32_t)(idx - row.rowoff);
#pragma unroll
                    for (int c = 0; c < 4; ++c) inter |= (labels[j + c] != li ? 1u : 0u) << c;
                }
            } else {
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    if (idx + c >= begin && idx + c < end) {
                        v[c] = vals[idx + c];
                        in |= 1u << c;
                        if (labels) inter |= (labels[row.colbase + (uint32_t)(idx + c - row.rowoff)] != li ? 1u : 0u) << c;
                    }
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const bool live = (in >> c) & 1u;
                uint32_t x = 0;
                if (live) x = hist_class(edges, n_edges, v[c], descending, last) + ((inter >> c) & 1u) * nclass;
                hist_count(cnt, x, live, lane);
            }
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < ncnt; t += 256) {
        const uint32_t x = cnt[t];
        if (x) (void)atomicAdd(out + t, (unsigned long long)x);
    }
}

}  // namespace

size_t hist_lds_bytes(uint32_t n_edges, int planes) { return ((size_t)n_edges + (size_t)planes * (n_edges + 2)) * sizeof(uint32_t); }

hipError_t launch_hist(hipStream_t st, const float *vals, const ThrRows &g, const float *d_edges, uint32_t n_edges, const uint32_t *labels,
                       int descending, uint32_t cus, uint64_t *counts)
{
    if (g.rows == 0) return hipSuccess;
    if (n_edges == 0 || n_edges > DSH_HIST_MAX_EDGES) return hipErrorInvalidValue;
    const size_t lds = hist_lds_bytes(n_edges, labels ? 2 : 1);
    const uint64_t units = g.rows * g.nchunks;
    const uint64_t grid = plan::hist_grid(units, lds, cus);
    if (grid > 0x7FFFFFFFull || (units + 4 * grid - 1) / (4 * grid) > plan::kHistMaxIters) return hipErrorInvalidValue;
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(k_hist), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_hist, dim3((uint32_t)grid), dim3(256), lds, st, vals, g, d_edges, n_edges, labels, descending, units,
                       reinterpret_cast<unsigned long long *>(counts));
    return hipGetLastError();
}

hipError_t preload_hist_kernels()
{
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_hist));
}

}  // namespace dsh
