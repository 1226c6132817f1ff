// kernels_exchange.hip -- the kernels of the multi-GPU exchange (exchange.hip): row placement of row-sorted parts at the
// destination, the older shard scheme's un-permute, and the two kernels of the one-GPU diagnostics.
#include <algorithm>

#include "kernels.h"

namespace dsh {

// row-sorted parts (plan.h): the rows at the positions [pos0, pos1) of a source rank's key order, lying at rowoff[s] of its
// buffer, go to their places in dashing's packed triangle (row r starts at r (2n - r - 1) / 2 and holds n - 1 - r values).
// A row is contiguous on both sides; a block copies kPlaceChunk values of it (blockIdx.y = the chunk: the longest rows
// of a part -- 40 KB at n = 10 000 -- would otherwise keep 128 blocks busy while 128 CUs idle).
constexpr uint32_t kPlaceChunk = 4096;
__device__ __forceinline__ void place_row_chunk(const float *__restrict__ src, float *__restrict__ out, const uint32_t *__restrict__ order,
                                                const uint64_t *__restrict__ rowoff, uint64_t s, uint64_t n)
{
    const uint64_t r = order[s], len = n - 1 - r;
    const uint64_t x0 = (uint64_t)blockIdx.y * kPlaceChunk;
    if (x0 >= len) return;
    const uint64_t x1 = x0 + kPlaceChunk < len ? x0 + kPlaceChunk : len;
    const float *from = src + rowoff[s];
    float *to = out + r * (2 * n - r - 1) / 2;
    for (uint64_t x = x0 + threadIdx.x; x < x1; x += 256) to[x] = from[x];
}

__global__ __launch_bounds__(256) void k_row_place(const float *__restrict__ src, float *__restrict__ out,
                                                    const uint32_t *__restrict__ order, const uint64_t *__restrict__ rowoff,
                                                    uint64_t pos0, uint64_t n)
{
    place_row_chunk(src, out, order, rowoff, pos0 + blockIdx.x, n);
}

hipError_t launch_row_place(hipStream_t st, const float *src, float *out, const uint32_t *order, const uint64_t *rowoff,
                            uint64_t pos0, uint64_t pos1, uint64_t n)
{
    if (pos1 <= pos0 || n < 2) return hipSuccess;
    hipLaunchKernelGGL(k_row_place, dim3((uint32_t)(pos1 - pos0), (uint32_t)((n - 1 + kPlaceChunk - 1) / kPlaceChunk)), dim3(256), 0, st,
                       src, out, order, rowoff, pos0, n);
    return hipGetLastError();
}

// one round of the exchange at the destination: the parts of ALL row-sorted sources that arrived in it, in ONE launch
// (a launch per source left seven small kernels in a row behind the last transfer of an 8-rank step).  Entry e covers
// the blocks [row0, row0 + nrows) of the grid's x.
__global__ __launch_bounds__(256) void k_rows_place(const PlaceEnt *__restrict__ ent, uint32_t nent, float *__restrict__ out, uint64_t n)
{
    uint32_t e = 0;
    while (e + 1 < nent && ent[e + 1].row0 <= blockIdx.x) ++e;
    const PlaceEnt E = ent[e];
    place_row_chunk(E.src, out, E.order, E.rowoff, E.pos0 + (blockIdx.x - E.row0), n);
}

hipError_t launch_rows_place(hipStream_t st, const PlaceEnt *ent, uint32_t nent, uint32_t total_rows, float *out, uint64_t n)
{
    if (!nent || !total_rows || n < 2) return hipSuccess;
    hipLaunchKernelGGL(k_rows_place, dim3(total_rows, (uint32_t)((n - 1 + kPlaceChunk - 1) / kPlaceChunk)), dim3(256), 0, st, ent, nent, out, n);
    return hipGetLastError();
}


// same mapping driven from the destination: one block per ORIGINAL row a, coalesced writes of
// row a of the output, gathered reads (inv = inverse of perm)
__global__ __launch_bounds__(256) void k_unpermute_gather(const float *__restrict__ in,
                                                           const uint32_t *__restrict__ inv, uint64_t n,
                                                           float *__restrict__ out)
{
    const uint64_t a = blockIdx.x;
    const uint64_t sa = inv[a];
    float *row = out + a * (2 * n - a - 1) / 2 - (a + 1);
    for (uint64_t b = a + 1 + threadIdx.x; b < n; b += 256) {
        const uint64_t sb = inv[b];
        const uint64_t lo = sa < sb ? sa : sb, hi = sa < sb ? sb : sa;
        row[b] = in[lo * (2 * n - lo - 1) / 2 + hi - (lo + 1)];
    }
}

// as k_unpermute_gather, but the spans of the shards sit at a fixed stride in `in` (the padded blocks an
// RCCL gather delivers): rowdelta[sorted row / 128] = shard * stride - span_off[shard]
__global__ __launch_bounds__(256) void k_unpermute_staged(const float *__restrict__ in,
                                                           const uint32_t *__restrict__ inv,
                                                           const int64_t *__restrict__ rowdelta,
                                                           uint64_t n, float *__restrict__ out)
{
    const uint64_t a = blockIdx.x;
    const uint64_t sa = inv[a];
    float *row = out + a * (2 * n - a - 1) / 2 - (a + 1);
    for (uint64_t b = a + 1 + threadIdx.x; b < n; b += 256) {
        const uint64_t sb = inv[b];
        const uint64_t lo = sa < sb ? sa : sb, hi = sa < sb ? sb : sa;
        row[b] = in[(int64_t)(lo * (2 * n - lo - 1) / 2 + hi - (lo + 1)) + rowdelta[lo / kTile]];
    }
}

hipError_t launch_unpermute_staged(hipStream_t st, const float *in, const uint32_t *inv,
                                   const int64_t *rowdelta, uint64_t n, float *out)
{
    if (n < 2) return hipSuccess;
    hipLaunchKernelGGL(k_unpermute_staged, dim3((uint32_t)(n - 1)), dim3(256), 0, st, in, inv, rowdelta, n, out);
    return hipGetLastError();
}

hipError_t launch_unpermute(hipStream_t st, const float *in, const uint32_t *inv, uint64_t n, float *out)
{
    if (n < 2) return hipSuccess;
    hipLaunchKernelGGL(k_unpermute_gather, dim3((uint32_t)(n - 1)), dim3(256), 0, st, in, inv, n, out);
    return hipGetLastError();
}

hipError_t preload_exchange_kernels()
{
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_row_place));
}

// ---- diagnostics of the exchange on ONE GPU (dsh_exchange_probe_parts_async, dsh_diag_spin_*) ---------------------------
namespace {

// what an RCCL send kernel does with a part: plain loads of the rank's buffer through the L2 of whatever XCD the
// workgroup runs on (NOT the copy engine, which reads memory), stores into another buffer
__global__ __launch_bounds__(256) void k_probe_copy(const float *__restrict__ src, float *__restrict__ dst, uint64_t cnt)
{
    for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < cnt; x += (uint64_t)gridDim.x * 256) dst[x] = src[x];
}

// a kernel that waits like an RCCL receive kernel whose peers have nothing to send yet: `threads` lanes per workgroup,
// `lds` bytes of LDS held, lane 0 polling a word of page-locked host memory; leaves when the word is set or after
// max_ticks of the device's wall clock (so that a host that never comes back cannot hang the GPU)
__global__ void k_diag_spin(const uint32_t *flag, unsigned long long max_ticks, uint32_t *touched)
{
    extern __shared__ uint32_t spin_lds[];
    if (threadIdx.x == 0) spin_lds[0] = blockIdx.x;
    __syncthreads();
    const unsigned long long t0 = wall_clock64();
    for (;;) {
        uint32_t v = 0;
        if (threadIdx.x == 0) v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        v = __shfl(v, 0);
        if (__syncthreads_or(v != 0 || wall_clock64() - t0 > max_ticks)) break;
        __builtin_amdgcn_s_sleep(8);
    }
    if (threadIdx.x == 0 && touched) atomicAdd(touched, spin_lds[0] + 1 - blockIdx.x);
}

}  // namespace

hipError_t launch_probe_copy(hipStream_t st, const float *src, float *dst, uint64_t cnt)
{
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((cnt + 255) / 256, 2048);
    hipLaunchKernelGGL(k_probe_copy, dim3(blocks), dim3(256), 0, st, src, dst, cnt);
    return hipGetLastError();
}

hipError_t launch_diag_spin(hipStream_t st, uint32_t nblocks, uint32_t threads, uint32_t lds_bytes, const uint32_t *flag, unsigned long long max_ticks)
{
    if (lds_bytes > 64 * 1024) {
        const hipError_t e = ensure_dynamic_lds((const void *)k_diag_spin, lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_diag_spin, dim3(nblocks), dim3(threads), std::max<uint32_t>(lds_bytes, 16), st, flag, max_ticks, (uint32_t *)nullptr);
    return hipGetLastError();
}

}  // namespace dsh
