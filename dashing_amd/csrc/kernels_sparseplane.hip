// kernels_sparseplane.hip -- the sparse outer planes of the compare path (plan.h, Tuning::sparse_planes).
//
// The top plane of a tile, C(T) = #{t : a_t < T and b_t < T}, is the AND of two planes that are 97-98 % ones.  With the
// complement sets U(v) = {t : a_t >= v},
//     C(v) = m - |U_i| - |U_j| + |U_i & U_j|,
// and the sets hold a few hundred of the 2^p positions.  A (tile, plane) the planner routes here is counted from them and
// stored into the C(v) block the tile kernel would have written, bit for bit; k_finalize does not know the difference.
//
// Per (block, plane) the call needs -- a SLAB -- two things are made from that plane's words of the bit-plane matrix
// (k_sparse_build; the words are (register < v), so their complement is the set):
//   table  bit j of a position's 128 bits: column j of the block is in the set there.  Word-major, [4 words][2^p positions],
//          up to p = 15; position-major, [2^p positions][4 words], at p = 16 (below);
//   lists  [128 rows][cap]           the positions of every sketch's set, 16-bit, in no particular order, and their number.
// A position's name is (plane word) * 32 + (bit of that word); nothing looks at which register that is, as in the tile
// kernel (k_transform's bit order).
// k_sparse_count, one workgroup per (tile, plane): lane (row, column word) walks the row's list, gathers the 32 column bits
// of every listed position and adds them into bit-sliced vertical counters through a carry-save tree (Harley-Seal, eight
// words a step): one lane step serves 32 pairs.  The counters are then read out column by column.
// Two placements of the table.  Gathered from global memory (k_sparse_count: position-major, the four lanes of a row read
// one 16-byte piece) the kernel is bound by its gathers -- 16 scattered pieces per wave instruction; at C3 an item costs
// 0.39 (top plane) to 0.64 (the one below) of a dense one (profiles/sparse1).  So up to p = 15 one word of the table -- 32
// columns, 2^p x 4 bytes: 64 KiB at p = 14 -- is staged in LDS by each of FOUR workgroups per item (k_sparse_count_lds),
// the four lanes of a row take a quarter of its list each and add their counters at the end.  At p = 16 a word is
// 256 KiB, more than a CU holds: the global placement stays, and there the sets are sparse enough for it to pay well.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace dsh {

namespace {

constexpr int kSpChunk = 16;     // plane words a wave of k_sparse_build takes
constexpr int kSpCounters = 11;  // counter words of k_sparse_count: sets up to 2047 (plan.h, kSparseCapMax)

// One wave per (slab, half of the block's 128 columns, chunk of kSpChunk plane words); lane = column.
__global__ __launch_bounds__(256) void k_sparse_build(const uint32_t *__restrict__ planes, uint32_t Npad, uint32_t W, uint64_t ncols,
                                                      const uint2 *__restrict__ slabs, uint32_t nslabs, uint32_t cap, int wordmajor,
                                                      uint32_t *__restrict__ tab, uint16_t *__restrict__ lists, uint32_t *__restrict__ len)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nch = W / kSpChunk;
    const uint64_t unit = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (unit >= (uint64_t)nslabs * 2 * nch) return;  // (wave-uniform)
    const uint32_t ch = (uint32_t)(unit % nch), h = (uint32_t)(unit / nch) & 1u, s = (uint32_t)(unit / (2 * (uint64_t)nch));
    const uint2 sl = slabs[s];  // {block, plane}
    const uint32_t row = h * 64 + lane;
    const uint64_t col = (uint64_t)sl.x * kTile + row;
    const uint32_t w0 = ch * kSpChunk;
    const uint32_t *src = planes + ((uint64_t)sl.y * W + w0) * Npad + col;
    // (a padding column's plane words are zero: it is in no set)
    const uint32_t real = col < ncols ? 0xFFFFFFFFu : 0u;
    uint32_t x[kSpChunk];
#pragma unroll
    for (int k = 0; k < kSpChunk; ++k) x[k] = ~src[(uint64_t)k * Npad] & real;
    // the table: the 32 x 64 bit transpose of every word, a ballot per bit; lane b keeps bit b's and stores it
    const uint64_t m = (uint64_t)W * 32;
    uint32_t *trow = tab + ((uint64_t)s * m + (uint64_t)w0 * 32 + lane) * 4 + 2 * h;       // position-major: [position][word]
    uint32_t *tcol = tab + ((uint64_t)s * 4 + 2 * h) * m + (uint64_t)w0 * 32 + (lane & 31u);  // word-major: [word][position]
#pragma unroll
    for (int k = 0; k < kSpChunk; ++k) {
        const uint32_t xx = x[k];
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (uint32_t b = 0; b < 32; ++b) {
            const unsigned long long bal = __ballot((xx >> b) & 1u);
            if (lane == b) {
                lo = (uint32_t)bal;
                hi = (uint32_t)(bal >> 32);
            }
        }
        if (wordmajor) {  // (lanes 32 .. 63 hold zeros: they get their copy of lane - 32's pair and write the second word)
            const uint32_t hi2 = __shfl(hi, (int)(lane & 31u), 64);
            tcol[(lane >> 5) * m + (uint64_t)k * 32] = lane < 32 ? lo : hi2;
        } else if (lane < 32) {
            *reinterpret_cast<uint2 *>(trow + (uint64_t)k * 32 * 4) = make_uint2(lo, hi);
        }
    }
    // the column's list: its slots from one atomic per chunk
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kSpChunk; ++k) mine += (uint32_t)__popc(x[k]);
    if (!mine) return;
    uint32_t slot = atomicAdd(&len[(uint64_t)s * kTile + row], mine);
    uint16_t *dst = lists + ((uint64_t)s * kTile + row) * cap;
#pragma unroll
    for (int k = 0; k < kSpChunk; ++k) {
        uint32_t xx = x[k];
        while (xx) {
            const uint32_t b = (uint32_t)__builtin_ctz(xx);
            xx &= xx - 1;
            if (slot < cap) dst[slot] = (uint16_t)((w0 + k) * 32 + b);  // (the planner's bound keeps every set inside cap)
            ++slot;
        }
    }
}

__device__ __forceinline__ void csa(uint32_t &h, uint32_t &l, uint32_t a, uint32_t b, uint32_t c)
{
    const uint32_t u = a ^ b;
    h = (a & b) | (u & c);
    l = u ^ c;
}

__device__ __forceinline__ void put32(uint16_t *dst, const uint32_t (&v)[32])
{
#pragma unroll
    for (int q = 0; q < 4; ++q)
        reinterpret_cast<uint4 *>(dst)[q] = make_uint4(v[8 * q] | (v[8 * q + 1] << 16), v[8 * q + 2] | (v[8 * q + 3] << 16),
                                                       v[8 * q + 4] | (v[8 * q + 5] << 16), v[8 * q + 6] | (v[8 * q + 7] << 16));
}
__device__ __forceinline__ void put32(uint32_t *dst, const uint32_t (&v)[32])
{
#pragma unroll
    for (int q = 0; q < 8; ++q) reinterpret_cast<uint4 *>(dst)[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// One workgroup per item {tile index in band, plane, slab of the row block, slab of the column block}; 512 lanes as
// (row, column word).  cap is a multiple of 8: a lane reads its list eight 16-bit positions at a time.
template <typename CT>
__global__ __launch_bounds__(512) void k_sparse_count(const uint4 *__restrict__ items, const uint32_t *__restrict__ tab,
                                                      const uint16_t *__restrict__ lists, const uint32_t *__restrict__ len, uint32_t cap,
                                                      uint32_t m, CT *__restrict__ cum, uint64_t nslots)
{
    __shared__ uint32_t lenj[kTile];
    const uint4 it = items[blockIdx.x];
    const uint32_t tid = threadIdx.x, r = tid >> 2, w = tid & 3u;
    if (tid < kTile) lenj[tid] = len[(uint64_t)it.w * kTile + tid];
    __syncthreads();
    const uint32_t li_all = len[(uint64_t)it.z * kTile + r];
    const uint32_t li = li_all < cap ? li_all : cap;
    const uint16_t *lp = lists + ((uint64_t)it.z * kTile + r) * cap;
    const uint32_t *tb = tab + (uint64_t)it.w * m * 4 + w;
    uint32_t c[kSpCounters];
#pragma unroll
    for (int b = 0; b < kSpCounters; ++b) c[b] = 0;
    for (uint32_t k0 = 0; k0 < li; k0 += 8) {
        const uint4 pk = *reinterpret_cast<const uint4 *>(lp + k0);
        const uint32_t pw[4] = {pk.x, pk.y, pk.z, pk.w};
        uint32_t x[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const bool valid = k0 + q < li;  // (behind the list's end: no gather from whatever the slot holds)
            const uint32_t pos = valid ? (pw[q >> 1] >> (16 * (q & 1))) & 0xFFFFu : 0u;
            const uint32_t v = tb[(uint64_t)pos * 4];
            x[q] = valid ? v : 0u;
        }
        uint32_t t0, t1, t2, t3, f0, f1, e;
        csa(t0, c[0], c[0], x[0], x[1]);
        csa(t1, c[0], c[0], x[2], x[3]);
        csa(f0, c[1], c[1], t0, t1);
        csa(t2, c[0], c[0], x[4], x[5]);
        csa(t3, c[0], c[0], x[6], x[7]);
        csa(f1, c[1], c[1], t2, t3);
        csa(e, c[2], c[2], f0, f1);
#pragma unroll
        for (int b = 3; b < kSpCounters; ++b) {  // the eights' carry ripples up
            const uint32_t carry = c[b] & e;
            c[b] ^= e;
            e = carry;
        }
    }
    // column cc of this lane's word: bit cc of every counter word
    const uint32_t base = m - li_all;
    uint32_t out[32];
#pragma unroll
    for (int cc = 0; cc < 32; ++cc) {
        uint32_t cnt = 0;
#pragma unroll
        for (int b = 0; b < kSpCounters; ++b) cnt |= ((c[b] >> cc) & 1u) << b;
        out[cc] = (base - lenj[w * 32 + cc] + cnt) & (sizeof(CT) == 2 ? 0xFFFFu : 0xFFFFFFFFu);
    }
    put32(cum + (uint64_t)it.y * nslots + (uint64_t)it.x * (kTile * kTile) + (uint64_t)r * kTile + w * 32, out);
}

// The LDS placement: workgroup g of a group of 32 takes item (g / 32) * 8 + g % 8 -- so that an item's launch position
// still names its XCD (plan.cpp) -- and column word (g / 8) % 4.  lds: [2^p] the word's table, then the 32 columns' set sizes.
template <typename CT>
__global__ __launch_bounds__(512) void k_sparse_count_lds(const uint4 *__restrict__ items, uint32_t nitems, const uint32_t *__restrict__ tabw,
                                                          const uint16_t *__restrict__ lists, const uint32_t *__restrict__ len, uint32_t cap,
                                                          uint32_t m, CT *__restrict__ cum, uint64_t nslots)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sp_lds[];
    const uint32_t g = blockIdx.x, item = (g >> 5) * 8 + (g & 7u), w = (g >> 3) & 3u;
    if (item >= nitems) return;  // (the whole workgroup, in front of the barrier)
    const uint4 it = items[item];
    const uint32_t tid = threadIdx.x, r = tid >> 2, q = tid & 3u;
    const uint4 *src = reinterpret_cast<const uint4 *>(tabw + ((uint64_t)it.w * 4 + w) * m);
    for (uint32_t i = tid; i < m / 4; i += 512) reinterpret_cast<uint4 *>(sp_lds)[i] = src[i];
    if (tid < 32) sp_lds[m + tid] = len[(uint64_t)it.w * kTile + w * 32 + tid];
    __syncthreads();
    const uint32_t li_all = len[(uint64_t)it.z * kTile + r];
    const uint32_t li = li_all < cap ? li_all : cap;
    const uint16_t *lp = lists + ((uint64_t)it.z * kTile + r) * cap;
    uint32_t c[kSpCounters];
#pragma unroll
    for (int b = 0; b < kSpCounters; ++b) c[b] = 0;
    for (uint32_t k0 = 8 * q; k0 < li; k0 += 32) {  // (lane q of the row's four: every fourth group of eight entries)
        const uint4 pk = *reinterpret_cast<const uint4 *>(lp + k0);
        const uint32_t pw[4] = {pk.x, pk.y, pk.z, pk.w};
        uint32_t x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool valid = k0 + j < li;  // (behind the list's end: no read at whatever the slot holds)
            const uint32_t pos = valid ? (pw[j >> 1] >> (16 * (j & 1))) & 0xFFFFu : 0u;
            const uint32_t v = sp_lds[pos];
            x[j] = valid ? v : 0u;
        }
        uint32_t t0, t1, t2, t3, f0, f1, e;
        csa(t0, c[0], c[0], x[0], x[1]);
        csa(t1, c[0], c[0], x[2], x[3]);
        csa(f0, c[1], c[1], t0, t1);
        csa(t2, c[0], c[0], x[4], x[5]);
        csa(t3, c[0], c[0], x[6], x[7]);
        csa(f1, c[1], c[1], t2, t3);
        csa(e, c[2], c[2], f0, f1);
#pragma unroll
        for (int b = 3; b < kSpCounters; ++b) {
            const uint32_t carry = c[b] & e;
            c[b] ^= e;
            e = carry;
        }
    }
    // the four lanes of a row add their counters: a bit-sliced adder, twice (every lane of the wave takes part)
#pragma unroll
    for (int d = 1; d <= 2; d <<= 1) {
        uint32_t carry = 0;
#pragma unroll
        for (int b = 0; b < kSpCounters; ++b) {
            const uint32_t o = __shfl_xor(c[b], d, 64);
            const uint32_t u = c[b] ^ o;
            const uint32_t sum = u ^ carry;
            carry = (c[b] & o) | (u & carry);
            c[b] = sum;
        }
    }
    if (q != 0) return;
    const uint32_t base = m - li_all;
    uint32_t out[32];
#pragma unroll
    for (int cc = 0; cc < 32; ++cc) {
        uint32_t cnt = 0;
#pragma unroll
        for (int b = 0; b < kSpCounters; ++b) cnt |= ((c[b] >> cc) & 1u) << b;
        out[cc] = (base - sp_lds[m + cc] + cnt) & (sizeof(CT) == 2 ? 0xFFFFu : 0xFFFFFFFFu);
    }
    put32(cum + (uint64_t)it.y * nslots + (uint64_t)it.x * (kTile * kTile) + (uint64_t)r * kTile + w * 32, out);
}

}  // namespace

hipError_t launch_sparse_build(hipStream_t st, const uint32_t *planes, uint32_t Npad, uint32_t W, uint64_t ncols, const uint2 *slabs,
                               uint32_t nslabs, uint32_t cap, int wordmajor, uint32_t *tab, uint16_t *lists, uint32_t *len)
{
    if (nslabs == 0) return hipSuccess;
    if (W < kSpChunk || W % kSpChunk || cap % 8) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(len, 0, (size_t)nslabs * kTile * sizeof(uint32_t), st);
    if (e != hipSuccess) return e;
    const uint64_t units = (uint64_t)nslabs * 2 * (W / kSpChunk);
    hipLaunchKernelGGL(k_sparse_build, dim3((uint32_t)((units + 3) / 4)), dim3(256), 0, st, planes, Npad, W, ncols, slabs, nslabs, cap,
                       wordmajor, tab, lists, len);
    return hipGetLastError();
}

hipError_t launch_sparse_count(hipStream_t st, int cum_bytes, const uint4 *items, uint32_t nitems, int wordmajor, const uint32_t *tab,
                               const uint16_t *lists, const uint32_t *len, uint32_t cap, uint32_t m, void *cum, uint64_t nslots)
{
    if (nitems == 0) return hipSuccess;
    if (cap % 8 || cap > 2047) return hipErrorInvalidValue;
    if (wordmajor) {
        if (m < 512 || m > (1u << 15)) return hipErrorInvalidValue;  // (a word of the table in a CU's LDS)
        const size_t lds = (size_t)m * 4 + 32 * 4;
        const uint32_t grid = (nitems + 7) / 8 * 32;
#define DSH_SPL(CT)                                                                                                                   \
    do {                                                                                                                              \
        const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(k_sparse_count_lds<CT>), lds);                          \
        if (e != hipSuccess) return e;                                                                                                \
        hipLaunchKernelGGL(k_sparse_count_lds<CT>, dim3(grid), dim3(512), lds, st, items, nitems, tab, lists, len, cap, m, (CT *)cum, nslots); \
    } while (0)
        if (cum_bytes == 2) DSH_SPL(uint16_t);
        else DSH_SPL(uint32_t);
#undef DSH_SPL
        return hipGetLastError();
    }
    if (cum_bytes == 2)
        hipLaunchKernelGGL(k_sparse_count<uint16_t>, dim3(nitems), dim3(512), 0, st, items, tab, lists, len, cap, m, (uint16_t *)cum, nslots);
    else
        hipLaunchKernelGGL(k_sparse_count<uint32_t>, dim3(nitems), dim3(512), 0, st, items, tab, lists, len, cap, m, (uint32_t *)cum, nslots);
    return hipGetLastError();
}

hipError_t preload_sparseplane_kernels()
{
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_sparse_build));
}

}  // namespace dsh
