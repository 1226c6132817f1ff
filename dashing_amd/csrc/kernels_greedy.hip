// kernels_greedy.hip -- greedy representatives at a threshold (greedy.hip): the lexicographically first
// maximal independent set of the hit graph in slot order, every other slot labelled with its first representative.
//
// assign is a uint32 [n] array in device memory that starts as assign[x] = x and only ever decreases: assign[x] < x means
// "x is covered by the representative assign[x]".  The bands of the triangle come in ascending row order, so when band
// [b0, b1) is reached every row below b0 has said all it has to say: assign[b0..b1) is final EXCEPT for what the band's
// own rows do to each other.
//   k_greedy_diag    settles that: ONE workgroup holds assign[b0..b1) in LDS and walks the band's rows in ascending order.
//                    A row whose entry is still itself is a representative: its in-band values (the columns (i, b1)) are
//                    tested and a passing column whose entry is still itself takes i -- rows ascend, so the first
//                    representative to reach a column is its smallest, and every column belongs to one thread: no
//                    atomics.  A covered row costs a read of LDS and no barrier; a representative row one barrier (and
//                    every batch of 16 rows two).  The loop visits every row once.  The entries go back to assign at the
//                    end.
//   k_greedy_band    the walk of thr_walk.h (ThrRows, one wave per 4096-value chunk of a row, one aligned float4 per lane
//                    per step, ragged edges value by value).  Now assign[b0..b1) is final: a wave
//                    whose row is covered returns at once, a representative's wave lowers assign[j] to i for every passing
//                    column j >= b1 (the in-band columns belong to k_greedy_diag and are skipped, whole chunks of them
//                    without a load).  atomicMin commutes: the result is the smallest representative whatever the order.
//                    The read in front of it only spares the atomic where nothing would change (assign[j] never grows, so
//                    a stale value errs towards one atomic too many).  Accesses to assign here are relaxed agent-scope
//                    atomics, as in UfDevice.  No loop depends on what another thread does.
//   k_greedy_labels  a launch of its own, after the last band: labels[x] = assign[x]; representatives counted with
//                    __ballot + popcount and one atomicAdd per wave
//
// dsh_greedy_extend* (greedy_extend.hip) adds three kernels; the three above are not changed.  Slots below
// m = first_new keep the labels the caller gives (assign[x] = labels_in[x]); in BEST mode best[n - m] holds, per new slot,
// the largest key of a representative that hits it -- 0: none; high word: the value as an order-preserving integer (the
// two zeros made one, complemented for the distances: a larger key is a better value); low word 0xFFFFFFFF - r: among equal
// values the smallest representative wins.  A plain 64-bit atomic maximum, which commutes like the minimum on assign.
//   k_greedy_rect    the geometry of k_greedy_band on the rows of a RECTANGLE (old rows [b0, b1) x the new columns [m, n),
//                    row r at r * ncols: any alignment mod 4): a wave whose old row is not a representative returns at once;
//                    a passing column is lowered in assign and, in BEST, raised in best
//   k_greedy_best    BEST only, in the place of k_greedy_band: the band's representative rows (final after k_greedy_diag)
//                    raise best for ALL their passing columns, the in-band ones included (a passing column of a
//                    representative row is never a representative: no test), and lower assign for the columns >= b1 as
//                    k_greedy_band does -- the band's out-of-band part is read once, its diagonal block a second time
//   k_greedy_extend_labels  labels[x] = assign[x] for old slots and in FIRST; in BEST a covered new slot takes the slot its
//                    key names; representatives counted as in k_greedy_labels
#include <hip/hip_runtime.h>

#include <algorithm>

#include "kernels.h"
#include "thr_walk.h"
#include "vkey.h"

namespace dsh {

namespace {

constexpr uint32_t kDiagThreads = 1024;
constexpr uint32_t kDiagCols = kGreedyMaxRows / kDiagThreads;  // band columns a thread of k_greedy_diag owns
constexpr uint32_t kDiagBatch = 16;                            // rows whose values it loads at once

__device__ __forceinline__ uint32_t ld_assign(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// rows <= kGreedyMaxRows (the host's band rule); one workgroup.  Thread t owns the band columns t, t + 1024, ...
// The rows are taken kDiagBatch at a time: first every thread loads, for the batch's rows that are still themselves, the
// values at its columns and keeps one pass bit per (row, column) -- the loads of a batch are independent of each other, so
// their latencies overlap instead of adding up row by row --, then the batch's rows are settled one after the other from
// the bits and LDS alone.  A row that was covered before its batch is neither loaded nor visited.
__global__ __launch_bounds__(kDiagThreads) void k_greedy_diag(const float *__restrict__ vals, ThrRows g, float t, int descending,
                                                               uint32_t *assign)
{
    __shared__ uint32_t cur[kGreedyMaxRows];
    const uint32_t rows = (uint32_t)g.rows, b0 = (uint32_t)g.row0;
    const uint64_t first = g.n - 1 - g.row0;  // values of the band's first row
    for (uint32_t r = threadIdx.x; r < rows; r += kDiagThreads) cur[r] = assign[g.row0 + r];
    for (uint32_t r0 = 0; r0 + 1 < rows; r0 += kDiagBatch) {  // (the band's last row has no in-band column)
        const uint32_t nb = rows - 1 - r0 < kDiagBatch ? rows - 1 - r0 : kDiagBatch;
        __syncthreads();  // every write of the batches before (and the load above) has landed
        uint32_t live = 0;  // rows of the batch that are still themselves: the same in every thread
#pragma unroll
        for (uint32_t rr = 0; rr < kDiagBatch; ++rr)
            if (rr < nb && cur[r0 + rr] == b0 + r0 + rr) live |= 1u << rr;
        __syncthreads();  // nobody writes before everybody has read
        if (!live) continue;
        uint32_t bits[kDiagCols];
        const uint64_t rowoff0 = band_rowoff(first, r0);
#pragma unroll
        for (uint32_t v = 0; v < kDiagCols; ++v) {
            bits[v] = 0;
            const uint32_t col = threadIdx.x + v * kDiagThreads;
            if (col >= rows || col <= r0) continue;
            // every load is issued, none under a branch (a value that is not wanted is read from vals[0] and dropped): the
            // compiler may then put all of them in flight before it waits for the first
            float x[kDiagBatch];
            uint64_t rowoff = rowoff0;
#pragma unroll
            for (uint32_t rr = 0; rr < kDiagBatch; ++rr) {
                const uint32_t r = r0 + rr;
                const bool want = ((live >> rr) & 1u) && col > r;
                x[rr] = vals[want ? rowoff + (col - r - 1) : 0];
                rowoff += first - r;  // row r + 1 starts behind the n - 1 - (row0 + r) values of row r
            }
#pragma unroll
            for (uint32_t rr = 0; rr < kDiagBatch; ++rr)
                if (((live >> rr) & 1u) && col > r0 + rr && thr_pass(x[rr], t, descending)) bits[v] |= 1u << rr;
        }
        for (uint32_t rr = 0; rr < nb; ++rr) {
            // cur[r] is settled: rows to the left of r wrote it before their barrier, rows to the right never do
            const uint32_t r = r0 + rr;
            if (!((live >> rr) & 1u) || cur[r] != b0 + r) continue;  // covered: before the batch, or by a row of it
#pragma unroll
            for (uint32_t v = 0; v < kDiagCols; ++v) {
                const uint32_t col = threadIdx.x + v * kDiagThreads;
                if (((bits[v] >> rr) & 1u) && cur[col] == b0 + col) cur[col] = b0 + r;
            }
            __syncthreads();
        }
    }
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < rows; r += kDiagThreads) assign[g.row0 + r] = cur[r];
}

// the walk of thr_walk.h, triangle rows only (thr_tri_row: launch_greedy_band takes no rectangle)
__global__ __launch_bounds__(256) void k_greedy_band(const float *__restrict__ vals, ThrRows g, float t, int descending, uint32_t *assign)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r = blockIdx.x;
    const uint32_t ch = blockIdx.y * 4 + wave;
    if (ch >= g.nchunks) return;
    const uint64_t i = g.row0 + r;
    const ThrRow row = thr_tri_row(g, r);
    const uint64_t inband = row.rowoff + (g.rows - 1 - r);  // behind the row's first values: the columns inside the band
    uint64_t begin, end;
    if (!thr_chunk(row, ch, begin, end) || end <= inband) return;  // past the row, or wholly inside the band's own columns
    if (ld_assign(assign + i) != (uint32_t)i) return;  // covered: the row has nothing to say
    if (begin < inband) begin = inband;
    for (uint64_t idx = thr_first(begin, lane); idx < end; idx += kThrStep) {
        float v[4];
        const uint32_t m = thr_flags(vals, idx, begin, end, t, descending, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!((m >> c) & 1u)) continue;
            uint32_t *a = assign + (row.colbase + (uint32_t)(idx + c - row.rowoff));
            if (ld_assign(a) > (uint32_t)i) (void)atomicMin(a, (uint32_t)i);
        }
    }
}

__global__ __launch_bounds__(256) void k_greedy_labels(const uint32_t *__restrict__ assign, uint64_t n, uint32_t *__restrict__ labels,
                                                       unsigned long long *n_reps)
{
    const uint64_t nround = (n + 255) / 256 * 256;  // whole waves take part in the ballot
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < nround; x += (uint64_t)gridDim.x * 256) {
        bool rep = false;
        if (x < n) {
            const uint32_t l = assign[x];
            labels[x] = l;
            rep = l == (uint32_t)x;
        }
        const unsigned long long b = __ballot(rep);
        if ((threadIdx.x & 63u) == 0 && b) atomicAdd(n_reps, (unsigned long long)__popcll(b));
    }
}

__device__ __forceinline__ unsigned long long ld_best(const unsigned long long *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// larger key = better value: the float's bits as an integer of the same order (-0.0 taken as +0.0 first, the bit-exact
// form of v + 0.0f: equal as float32 must mean equal here), complemented where a smaller value is better; NaN never passes
__device__ __forceinline__ unsigned long long best_key(float v, int descending, uint32_t r)
{
    return ((unsigned long long)value_key32(v, descending) << 32) | (unsigned long long)(0xFFFFFFFFu - r);
}

// One wave, one chunk [begin, end) of the values of representative row i: a passing column j is lowered in assign if
// j >= min_from, and raised in best (if there is one).
__device__ __forceinline__ void greedy_walk(const float *__restrict__ vals, const ThrRow row, uint64_t begin, uint64_t end, uint32_t i, uint32_t lane,
                                            float t, int descending, uint32_t *assign, uint32_t min_from, unsigned long long *best, uint32_t m)
{
    for (uint64_t idx = thr_first(begin, lane); idx < end; idx += kThrStep) {
        float v[4];
        const uint32_t hit = thr_flags(vals, idx, begin, end, t, descending, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (!((hit >> c) & 1u)) continue;
            const uint32_t j = row.colbase + (uint32_t)(idx + c - row.rowoff);
            if (j >= min_from) {
                uint32_t *a = assign + j;
                if (ld_assign(a) > i) (void)atomicMin(a, i);
            }
            if (best) {
                unsigned long long *b = best + (j - m);
                const unsigned long long key = best_key(v[c], descending, i);
                if (ld_best(b) < key) (void)atomicMax(b, key);  // (best only grows: a stale value errs towards one atomic too many)
            }
        }
    }
}

// g.rect = 1: rows [g.row0, g.row0 + g.rows) of the collection against the columns [g.col0, g.col0 + g.ncols) = [m, n)
__global__ __launch_bounds__(256) void k_greedy_rect(const float *__restrict__ vals, ThrRows g, float t, int descending, uint32_t *assign,
                                                     unsigned long long *best)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r = blockIdx.x;
    const uint32_t ch = blockIdx.y * 4 + wave;
    if (ch >= g.nchunks) return;
    const ThrRow row = thr_rect_row(g, r);
    uint64_t begin, end;
    if (!thr_chunk(row, ch, begin, end)) return;
    const uint64_t i = g.row0 + r;
    if (ld_assign(assign + i) != (uint32_t)i) return;  // not a representative: the row has nothing to say
    greedy_walk(vals, row, begin, end, (uint32_t)i, lane, t, descending, assign, 0u, best, (uint32_t)g.col0);
}

// a band of triangle rows as k_greedy_band takes it (thr_tri_row: launch_greedy_best takes no rectangle), after k_greedy_diag;
// m <= g.row0
__global__ __launch_bounds__(256) void k_greedy_best(const float *__restrict__ vals, ThrRows g, float t, int descending, uint32_t *assign,
                                                     unsigned long long *best, uint32_t m)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t r = blockIdx.x;
    const uint32_t ch = blockIdx.y * 4 + wave;
    if (ch >= g.nchunks) return;
    const uint64_t i = g.row0 + r;
    if (!thr_chunk_inside(g.n - 1 - i, ch)) return;  // past the row
    if (ld_assign(assign + i) != (uint32_t)i) return;  // covered
    const ThrRow row = thr_tri_row(g, r);  // (behind the load, as the kernel was written: its register count depends on it)
    uint64_t begin, end;
    (void)thr_chunk(row, ch, begin, end);
    greedy_walk(vals, row, begin, end, (uint32_t)i, lane, t, descending, assign, (uint32_t)(g.row0 + g.rows), best, m);
}

__global__ __launch_bounds__(256) void k_greedy_extend_labels(const uint32_t *__restrict__ assign, const unsigned long long *__restrict__ best,
                                                              uint64_t m, uint64_t n, uint32_t *__restrict__ labels,
                                                              unsigned long long *n_reps)
{
    const uint64_t nround = (n + 255) / 256 * 256;  // whole waves take part in the ballot
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < nround; x += (uint64_t)gridDim.x * 256) {
        bool rep = false;
        if (x < n) {
            uint32_t l = assign[x];
            if (best && x >= m && l != (uint32_t)x) l = 0xFFFFFFFFu - (uint32_t)best[x - m];
            labels[x] = l;
            rep = l == (uint32_t)x;
        }
        const unsigned long long b = __ballot(rep);
        if ((threadIdx.x & 63u) == 0 && b) atomicAdd(n_reps, (unsigned long long)__popcll(b));
    }
}

}  // namespace

hipError_t launch_greedy_diag(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *assign)
{
    if (g.rows < 2 || g.rect) return hipSuccess;  // (one row has no in-band column)
    if (g.rows > kGreedyMaxRows) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_greedy_diag, dim3(1), dim3(kDiagThreads), 0, st, vals, g, t, descending, assign);
    return hipGetLastError();
}

hipError_t launch_greedy_band(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *assign)
{
    if (g.rows == 0 || g.rect) return hipSuccess;
    hipLaunchKernelGGL(k_greedy_band, thr_grid(g), dim3(256), 0, st, vals, g, t, descending, assign);
    return hipGetLastError();
}

hipError_t launch_greedy_labels(hipStream_t st, const uint32_t *assign, uint64_t n, uint32_t *labels, uint64_t *n_reps)
{
    if (!n) return hipSuccess;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 8192);
    hipLaunchKernelGGL(k_greedy_labels, dim3(grid), dim3(256), 0, st, assign, n, labels, reinterpret_cast<unsigned long long *>(n_reps));
    return hipGetLastError();
}

hipError_t launch_greedy_rect(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *assign, uint64_t *best)
{
    if (g.rows == 0 || g.ncols == 0) return hipSuccess;
    if (!g.rect) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_greedy_rect, thr_grid(g), dim3(256), 0, st, vals, g, t, descending, assign,
                       reinterpret_cast<unsigned long long *>(best));
    return hipGetLastError();
}

hipError_t launch_greedy_best(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *assign, uint64_t *best,
                              uint64_t first_new)
{
    if (g.rows == 0) return hipSuccess;
    if (g.rect || !best || first_new > g.row0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_greedy_best, thr_grid(g), dim3(256), 0, st, vals, g, t, descending, assign,
                       reinterpret_cast<unsigned long long *>(best), (uint32_t)first_new);
    return hipGetLastError();
}

hipError_t launch_greedy_extend_labels(hipStream_t st, const uint32_t *assign, const uint64_t *best, uint64_t first_new, uint64_t n,
                                       uint32_t *labels, uint64_t *n_reps)
{
    if (!n) return hipSuccess;
    const uint32_t grid = (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + 255) / 256, 1), 8192);
    hipLaunchKernelGGL(k_greedy_extend_labels, dim3(grid), dim3(256), 0, st, assign, reinterpret_cast<const unsigned long long *>(best),
                       first_new, n, labels, reinterpret_cast<unsigned long long *>(n_reps));
    return hipGetLastError();
}

}  // namespace dsh
