// kernels_dbscan.hip -- density clusters at a threshold (dbscan.hip; include/dashing_hip.h has the
// contract).  G is the graph of the values that pass the threshold (thr_pass, NaN never).  Two walks over the dense bands, each
// band walked as thr_walk.h lays down, and a labelling pass; every kernel is a launch of its own, so that what the one
// before wrote is visible.
//
// Walk 1, degree[x] = the edges at x.  The number of atomics does not grow with the hits (the pattern of kernels_group.hip):
//   k_db_deg_rows  one wave per 4096-value chunk of a row, one aligned float4 per lane per step, ragged edges value by value;
//                  the hits are counted with __ballot + popcount and the wave issues ONE atomicAdd into degree[i], none for a
//                  chunk without a hit
//   k_db_deg_cols  the band's contribution to its COLUMNS: a thread owns column j and walks the rows i < j of one slab of
//                  kDbSlab band rows (consecutive threads read consecutive addresses of a row), counts privately and issues
//                  one atomicAdd per (column, slab) that saw a hit
// Walk 2 (degree[] is final: x is a core iff degree[x] + 1 >= min_pts, compared in 64 bits):
//   k_db_band      the geometry of k_cc_band.  The row's core flag and root are found once per chunk.  A passing value at
//                  column j: both ends cores -> the step of k_cc_band (find(j), skip on equal roots, else unite; uf_dev.h);
//                  exactly one end a core c -> the key (hi << 32 | ~c) is offered to best[the other end] under a 64-bit maximum,
//                  hi = value_key32(v) for BEST and 1 for FIRST, so the largest key names the best value and, on equal values, the
//                  smallest core; 0 = no core neighbour (~c >= 1 since n <= 2^32 - 1).  Row side: the lanes keep their largest
//                  key in a register, the wave reduces it and issues at most ONE atomicMax per chunk.  Column side: best[j] is
//                  read first and the atomicMax issued only for a larger key (best only grows: a stale read costs a redundant
//                  atomic and never loses an update).  A non-core has at most min_pts - 2 edges, so the offers are bounded by
//                  n (min_pts - 2) whatever the threshold.  Neither end a core: nothing.  Nothing is united through a non-core.
//   k_db_labels    core: find(x); border (best[x] != 0): find(~low32(best[x])); noise: x.  kind, and degree where asked, are
//                  written beside; clusters (cores that are their own label) and noise are counted with __ballot + popcount
//                  and one 64-bit atomicAdd per wave each.  A NULL optional output is not written.
// Every loop is bounded (uf.h: cap); no thread waits for another.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/dashing_hip.h"
#include "kernels.h"
#include "thr_walk.h"
#include "uf_dev.h"
#include "vkey.h"

namespace dsh {

namespace {

__device__ __forceinline__ bool db_core(uint32_t degree, uint32_t min_pts) { return (uint64_t)degree + 1 >= (uint64_t)min_pts; }

__device__ __forceinline__ uint64_t db_load64(const uint64_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// an offer to the non-core x
__device__ __forceinline__ void db_offer(uint64_t *best, uint32_t x, uint64_t w)
{
    if (db_load64(best + x) < w) (void)atomicMax((unsigned long long *)(best + x), (unsigned long long)w);
}

__device__ __forceinline__ uint64_t db_key(float v, int descending, int assign_best, uint32_t core)
{
    const uint32_t hi = assign_best ? value_key32(v, descending) : 1u;
    return (uint64_t)hi << 32 | (uint32_t)~core;
}

// The walk of thr_walk.h, triangle rows only (thr_tri_row: launch_db_degree takes no rectangle).
__global__ __launch_bounds__(256) void k_db_deg_rows(const float *__restrict__ vals, ThrRows g, float t, int descending, uint32_t *degree)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r = blockIdx.x;
    const uint32_t ch = blockIdx.y * 4 + wave;
    if (ch >= g.nchunks) return;  // (the whole wave)
    const uint64_t i = g.row0 + r;
    const ThrRow row = thr_tri_row(g, r);
    uint64_t begin, end;
    if (!thr_chunk(row, ch, begin, end)) return;
    uint32_t hits = 0;
    // every lane takes every step (the ballots see whole waves); a lane behind the chunk's end loads nothing and flags nothing
    for (uint64_t base = begin & ~(uint64_t)3; base < end; base += kThrStep) {  // at most kThrChunk / kThrStep + 1 steps
        float v[4];
        const uint32_t m = thr_flags(vals, base + 4 * lane, begin, end, t, descending, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) hits += (uint32_t)__popcll(__ballot((m >> c) & 1u));
    }
    if (lane == 0 && hits) (void)atomicAdd(degree + i, hits);
}

// block (x, y): the slab y of band rows [y kDbSlab, ...) and the 256 columns from the slab's first row + 1 + 256 x on
__global__ __launch_bounds__(256) void k_db_deg_cols(const float *__restrict__ vals, ThrRows g, float t, int descending, uint32_t *degree)
{
    const uint64_t r0 = (uint64_t)blockIdx.y * kDbSlab;
    if (r0 >= g.rows) return;
    const uint64_t r1 = r0 + kDbSlab < g.rows ? r0 + kDbSlab : g.rows;
    const uint64_t j = g.row0 + r0 + 1 + (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= g.n) return;
    const uint64_t first = g.n - 1 - g.row0;
    uint64_t off = band_rowoff(first, r0);  // start of band row r0, then of each next one
    const uint64_t rend = j - g.row0 < r1 ? j - g.row0 : r1;  // rows i < j only
    uint32_t hits = 0;
    for (uint64_t r = r0; r < rend; ++r) {  // at most kDbSlab steps
        hits += thr_pass(vals[off + (j - (g.row0 + r) - 1)], t, descending) ? 1u : 0u;
        off += first - r;
    }
    if (hits) (void)atomicAdd(degree + j, hits);
}

__global__ __launch_bounds__(256) void k_db_band(const float *__restrict__ vals, ThrRows g, float t, int descending,
                                                 const uint32_t *__restrict__ degree, uint32_t min_pts, int assign_best, uint32_t *parent,
                                                 uint32_t cap, uint32_t *err, uint64_t *best)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r = blockIdx.x;
    const uint32_t ch = blockIdx.y * 4 + wave;
    if (ch >= g.nchunks) return;  // (the whole wave)
    const uint32_t i = (uint32_t)(g.row0 + r);
    const ThrRow row = thr_tri_row(g, r);
    uint64_t begin, end;
    if (!thr_chunk(row, ch, begin, end)) return;
    const bool core_i = db_core(degree[i], min_pts);
    // a core row's root is kept for the whole chunk (every lane its own copy) and refreshed after a hook, as in k_cc_band
    uint32_t root_i = core_i ? uf_find<UfDevice>(parent, i, cap) : i;
    bool lost = root_i == kUfOverrun, bad = lost;  // a find ran over its bound; the lane stops
    uint64_t mine = 0;  // the lane's largest key for a non-core row i
    for (uint64_t idx = thr_first(begin, lane); idx < end && !bad; idx += kThrStep) {
        float v[4];
        const uint32_t m = thr_flags(vals, idx, begin, end, t, descending, v);
        if (!m) continue;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!((m >> c) & 1u) || bad) continue;  // (a flag is only set inside [begin, end): j is a column of the row, j < n)
            const uint32_t j = row.colbase + (uint32_t)(idx + c - row.rowoff);
            const bool core_j = db_core(degree[j], min_pts);
            if (core_i && core_j) {
                const uint32_t rj = uf_find<UfDevice>(parent, j, cap);
                if (rj == root_i) continue;  // the common case at loose thresholds: nothing to write
                if (rj == kUfOverrun) {
                    bad = lost = true;
                    continue;
                }
                root_i = cc_unite(parent, root_i, rj, cap, err);  // (stores its own code on an overrun)
                bad = root_i == kUfOverrun;
            } else if (core_i) {
                db_offer(best, j, db_key(v[c], descending, assign_best, i));
            } else if (core_j) {
                const uint64_t w = db_key(v[c], descending, assign_best, j);
                mine = w > mine ? w : mine;
            }
        }
    }
    if (lost) __hip_atomic_store(err, kUfErrFind, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (the call fails: what follows is moot)
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)mine, s);
        mine = o > mine ? o : mine;
    }
    if (lane == 0 && mine) db_offer(best, i, mine);
}

__global__ __launch_bounds__(256) void k_db_labels(uint32_t *parent, uint64_t n, uint32_t cap, const uint32_t *__restrict__ degree,
                                                   const uint64_t *__restrict__ best, uint32_t min_pts, uint32_t *__restrict__ labels,
                                                   uint8_t *__restrict__ kind_out, uint32_t *__restrict__ degree_out,
                                                   unsigned long long *n_clusters, unsigned long long *n_noise, uint32_t *err)
{
    const uint64_t nround = (n + 255) / 256 * 256;  // whole waves take part in the ballots
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < nround; x += (uint64_t)gridDim.x * 256) {
        bool head = false, noise = false;
        if (x < n) {
            const uint32_t d = degree[x];
            const uint64_t w = best[x];
            const bool core = db_core(d, min_pts);
            uint32_t l = (uint32_t)x;
            uint8_t kind = DSH_DBSCAN_NOISE;
            if (core || w) {
                kind = core ? DSH_DBSCAN_CORE : DSH_DBSCAN_BORDER;
                const uint32_t from = core ? (uint32_t)x : ~(uint32_t)w;
                l = from < n ? uf_find<UfDevice>(parent, from, cap) : kUfOverrun;  // (an offer names a core: a slot below n)
                if (l == kUfOverrun) {
                    __hip_atomic_store(err, kUfErrFind, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    l = (uint32_t)x;
                }
            }
            labels[x] = l;
            if (kind_out) kind_out[x] = kind;
            if (degree_out) degree_out[x] = d;
            head = core && l == (uint32_t)x;
            noise = kind == DSH_DBSCAN_NOISE;
        }
        const unsigned long long bh = __ballot(head), bn = __ballot(noise);
        if ((threadIdx.x & 63u) == 0) {
            if (bh) atomicAdd(n_clusters, (unsigned long long)__popcll(bh));
            if (bn) atomicAdd(n_noise, (unsigned long long)__popcll(bn));
        }
    }
}

}  // namespace

hipError_t launch_db_degree(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *degree)
{
    if (g.rows == 0 || g.rect || g.n < 2 || g.row0 + 1 >= g.n) return hipSuccess;
    const uint64_t colblocks = (g.n - 1 - g.row0 + 255) / 256, slabs = (g.rows + kDbSlab - 1) / kDbSlab;
    if (slabs > 65535) return hipErrorInvalidValue;  // (a band holds at most 2^20 rows: 2048 slabs)
    hipLaunchKernelGGL(k_db_deg_rows, thr_grid(g), dim3(256), 0, st, vals, g, t, descending, degree);
    hipLaunchKernelGGL(k_db_deg_cols, dim3((uint32_t)colblocks, (uint32_t)slabs), dim3(256), 0, st, vals, g, t, descending, degree);
    return hipGetLastError();
}

hipError_t launch_db_band(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, const uint32_t *degree,
                          uint32_t min_pts, int assign_best, uint32_t *parent, uint32_t cap, uint32_t *err, uint64_t *best)
{
    if (g.rows == 0 || g.rect) return hipSuccess;
    hipLaunchKernelGGL(k_db_band, thr_grid(g), dim3(256), 0, st, vals, g, t, descending, degree, min_pts, assign_best, parent, cap, err, best);
    return hipGetLastError();
}

hipError_t launch_db_labels(hipStream_t st, uint32_t *parent, uint64_t n, uint32_t cap, const uint32_t *degree, const uint64_t *best,
                            uint32_t min_pts, uint32_t *labels, uint8_t *kind_out, uint32_t *degree_out, uint64_t *n_clusters,
                            uint64_t *n_noise, uint32_t *err)
{
    if (!n) return hipSuccess;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((n + 255) / 256, 8192);
    hipLaunchKernelGGL(k_db_labels, dim3(grid), dim3(256), 0, st, parent, n, cap, degree, best, min_pts, labels, kind_out, degree_out,
                       reinterpret_cast<unsigned long long *>(n_clusters), reinterpret_cast<unsigned long long *>(n_noise), err);
    return hipGetLastError();
}

}  // namespace dsh
