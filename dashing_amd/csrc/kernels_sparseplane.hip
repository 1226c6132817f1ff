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
// 0.39 (top plane) to 0.64 (the one below) of a dense one (profiles/sparse1).  So up to p = 15 the table is staged in LDS
// (k_sparse_count_lds), NW = 1 or 2 of its words -- 32 columns each, 2^p x 4 bytes: 64 KiB at p = 14 -- by each of 4 / NW
// workgroups per item (option sparse_words; 2 where the pair fits a CU's 160 KiB beside the turn area, p <= 14, else 1).
// The 4 NW lanes of a row take every (4 NW)th group of eight entries of its list, add their counters at the end and read
// out eight of the 32 NW columns each.  The walk was bound by its LDS gathers: the lanes of a wave read random positions,
// which conflict on the banks; a 64-bit read of an interleaved word pair meets the same conflicts and returns twice the
// columns, so at NW = 2 a list entry costs half the LDS cycles per column, and the lists are read by half as many
// workgroups.  A workgroup takes a RUN of items of its XCD residue (option sparse_run, default plan::kSparseRunDefault)
// and stages its words again only where the table slab changes (profiles/sparse3, profiles/sparse4).  At p = 16 a word is
// 256 KiB, more than a CU holds: the global placement stays, and there the sets are sparse enough for it to pay well.
// The sided route (plan.h, Tuning::sparse_sided).  Only the LIST side has to be sparse -- the table costs the same at any
// density -- and a set may be U(v) or A(v) = {t : a_t < v}, the plane's words as they are: a slab carries its polarity, an
// item the polarities of its two sides, and C(v) comes from cnt = |R_list & S_table| by one of four formulas (sp_values).
// An item whose sparse side is the COLUMN block is transposed: the lanes walk the column block's lists against the row
// block's table, a lane then owns one column and 32 rows, and the values are turned through LDS before they are stored.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "kernels.h"
#include "plan.h"

namespace dsh {

namespace {

using plan::kSpItemListA;
using plan::kSpItemTabA;
using plan::kSpItemTransposed;
using plan::kSpPlaneMask;
using plan::kSpSlabA;
using plan::kSpSlabTableOnly;

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
    const uint2 sl = slabs[s];  // {block, plane | kSpSlab* flags}
    const uint32_t plane = sl.y & kSpPlaneMask;
    const uint32_t flip = sl.y & kSpSlabA ? 0u : 0xFFFFFFFFu;  // (the words are A(v); their complement is U(v))
    const uint32_t row = h * 64 + lane;
    const uint64_t col = (uint64_t)sl.x * kTile + row;
    const uint32_t w0 = ch * kSpChunk;
    const uint32_t *src = planes + ((uint64_t)plane * W + w0) * Npad + col;
    // (a padding column's plane words are zero: it is in no set of either polarity)
    const uint32_t real = col < ncols ? 0xFFFFFFFFu : 0u;
    uint32_t x[kSpChunk];
#pragma unroll
    for (int k = 0; k < kSpChunk; ++k) x[k] = (src[(uint64_t)k * Npad] ^ flip) & real;
    // The table: every word's bits turned, 32 lanes x 32 bits at a time in either half of the wave, by five rounds of lane
    // exchanges (blocks of j x j bits swap across lanes j apart, j = 16 .. 1): lane b of a half then holds bit b of its 32
    // columns -- a word of position w0 * 32 + k * 32 + b -- and stores it.  (A ballot per bit took five times the instructions.)
    const uint64_t m = (uint64_t)W * 32;
    const uint32_t q = 2 * h + (lane >> 5), b5 = lane & 31u;  // the table word this lane's half fills; the position in the plane word
    uint32_t *tpos = tab + ((uint64_t)s * m + (uint64_t)w0 * 32 + b5) * 4 + q;  // position-major: [position][word]
    uint32_t *tcol = tab + ((uint64_t)s * 4 + q) * m + (uint64_t)w0 * 32 + b5;  // word-major: [word][position]
#pragma unroll
    for (int k = 0; k < kSpChunk; ++k) {
        uint32_t t = x[k];
#pragma unroll
        for (uint32_t j = 16, mk = 0x0000FFFFu; j; j >>= 1, mk ^= mk << j) {  // mk: the bits whose index has bit j clear
            const uint32_t o = __shfl_xor(t, (int)j, 64);
            t = lane & j ? (t & ~mk) | ((o >> j) & mk) : (t & mk) | ((o & mk) << j);
        }
        if (wordmajor) tcol[(uint64_t)k * 32] = t;
        else tpos[(uint64_t)k * 32 * 4] = t;
    }
    // the column's list: its slots from one atomic per chunk
    uint32_t mine = 0;
#pragma unroll
    for (int k = 0; k < kSpChunk; ++k) mine += (uint32_t)__popc(x[k]);
    if (!mine) return;
    uint32_t slot = atomicAdd(&len[(uint64_t)s * kTile + row], mine);  // (the true size of the set: the formulas read it)
    if (sl.y & kSpSlabTableOnly) return;                               // (wave-uniform: no item walks this slab's lists)
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

// A lane's N values from its counter words, for the table columns c0 .. c0 + N - 1 of the word: bit cc of every word is
// cnt = |R & S| of the lane's list row against table column cc.  With the list set's size ll and the table set's size
// lt[j] of column c0 + j, by the polarities of the item's flags fl:
//     list U, table U: m - ll - lt + cnt     list A, table A: cnt     list U, table A: lt - cnt     list A, table U: ll - cnt
template <typename CT, int N>
__device__ __forceinline__ void sp_values(uint32_t (&out)[N], const uint32_t (&c)[kSpCounters], uint32_t c0, uint32_t fl, uint32_t m,
                                          uint32_t ll, const uint32_t *lt)
{
    const bool la = (fl & kSpItemListA) != 0, ta = (fl & kSpItemTabA) != 0;  // (wave-uniform: per item)
    const uint32_t kl = !la && !ta ? m - ll : la && !ta ? ll : 0u;
    const uint32_t tsub = !la && !ta ? 0xFFFFFFFFu : 0u, tadd = !la && ta ? 0xFFFFFFFFu : 0u;  // the table set's size: minus | plus | not at all
    const uint32_t cneg = la != ta ? 0xFFFFFFFFu : 0u;                                           // cnt: minus | plus
    uint32_t cs[kSpCounters];
#pragma unroll
    for (int b = 0; b < kSpCounters; ++b) cs[b] = c[b] >> c0;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        uint32_t cnt = 0;
#pragma unroll
        for (int b = 0; b < kSpCounters; ++b) cnt |= ((cs[b] >> j) & 1u) << b;
        const uint32_t t = lt[j];
        out[j] = (kl + (t & tadd) - (t & tsub) + ((cnt ^ cneg) - cneg)) & (sizeof(CT) == 2 ? 0xFFFFu : 0xFFFFFFFFu);
    }
}

// A transposed item's 32 x 128 values, staged as st[row][column] words, stored as whole rows by the workgroup's 512 lanes:
// dst = the first of the 32 rows in the tile's C(v) block.
template <typename CT>
__device__ __forceinline__ void sp_store_rows(const uint32_t *st, CT *dst, uint32_t tid)
{
    if (sizeof(CT) == 2) {
        const uint32_t at = (tid >> 4) * kTile + (tid & 15u) * 8;
        const uint4 a = *reinterpret_cast<const uint4 *>(st + at), b = *reinterpret_cast<const uint4 *>(st + at + 4);
        *reinterpret_cast<uint4 *>(dst + at) = make_uint4(a.x | (a.y << 16), a.z | (a.w << 16), b.x | (b.y << 16), b.z | (b.w << 16));
    } else {
#pragma unroll
        for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t g = tid + 512 * h, at = (g >> 5) * kTile + (g & 31u) * 4;
            *reinterpret_cast<uint4 *>(dst + at) = *reinterpret_cast<const uint4 *>(st + at);
        }
    }
}

// One workgroup per item {tile index in band, plane | kSpItem* flags, slab of the row block, slab of the column block}; 512
// lanes as (list row, table word).  cap is a multiple of 8: a lane reads its list eight 16-bit positions at a time.
template <typename CT>
__global__ __launch_bounds__(512) void k_sparse_count(const uint4 *__restrict__ items, const uint32_t *__restrict__ tab,
                                                      const uint16_t *__restrict__ lists, const uint32_t *__restrict__ len, uint32_t cap,
                                                      uint32_t m, CT *__restrict__ cum, uint64_t nslots)
{
    __shared__ uint32_t lenj[kTile];
    __shared__ __attribute__((aligned(16))) uint32_t turn[32 * kTile];  // (transposed items) 32 rows of the tile on their way out
    const uint4 it = items[blockIdx.x];
    const bool tr = (it.y & kSpItemTransposed) != 0;  // (uniform over the workgroup)
    const uint32_t ls = tr ? it.w : it.z, ts = tr ? it.z : it.w, plane = it.y & kSpPlaneMask;  // list slab, table slab
    const uint32_t tid = threadIdx.x, r = tid >> 2, w = tid & 3u;
    if (tid < kTile) lenj[tid] = len[(uint64_t)ts * kTile + tid];
    __syncthreads();
    const uint32_t li_all = len[(uint64_t)ls * kTile + r];
    const uint32_t li = li_all < cap ? li_all : cap;
    const uint16_t *lp = lists + ((uint64_t)ls * kTile + r) * cap;
    const uint32_t *tb = tab + (uint64_t)ts * m * 4 + w;
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
    uint32_t out[32];
    sp_values<CT, 32>(out, c, 0u, it.y, m, li_all, lenj + w * 32);
    CT *blk = cum + (uint64_t)plane * nslots + (uint64_t)it.x * (kTile * kTile);
    if (!tr) {
        put32(blk + (uint64_t)r * kTile + w * 32, out);
        return;
    }
    // transposed: lane (r, w) holds column r of the rows w * 32 .. w * 32 + 31; a quarter of the tile at a time
    for (uint32_t k = 0; k < 4; ++k) {
        if (w == k) {
#pragma unroll
            for (int cc = 0; cc < 32; ++cc) turn[cc * kTile + r] = out[cc];
        }
        __syncthreads();
        sp_store_rows<CT>(turn, blk + (uint64_t)k * 32 * kTile, tid);
        __syncthreads();
    }
}

__device__ __forceinline__ void put8(uint16_t *dst, const uint32_t (&v)[8])
{
    *reinterpret_cast<uint4 *>(dst) = make_uint4(v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16));
}
__device__ __forceinline__ void put8(uint32_t *dst, const uint32_t (&v)[8])
{
    reinterpret_cast<uint4 *>(dst)[0] = make_uint4(v[0], v[1], v[2], v[3]);
    reinterpret_cast<uint4 *>(dst)[1] = make_uint4(v[4], v[5], v[6], v[7]);
}

// The carry-save adder of the LDS placement as sum and majority, one v_bitop3_b32 each (truth tables 0x96, 0xE8).  Through
// the builtin: written with &, | and ^ the compiler rebuilds it from v_xor and v_bfi, four to five instructions an adder.
// (csa above stays as the gathered kernel has it.)
__device__ __forceinline__ void csa_sm(uint32_t &h, uint32_t &l, uint32_t a, uint32_t b, uint32_t c)
{
    h = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);
    l = __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// The gathers of one step of a lane's walk against the NW table words in LDS: the eight 16-bit positions of pk, of which
// `left` are in the list (kPartial: fewer than eight may be -- behind the list's end nothing is read at whatever the slot
// holds, and the words are zero).
template <int NW, bool kPartial>
__device__ __forceinline__ void sp_gather(uint32_t (&x)[NW][8], const uint32_t *tabl, const uint4 pk, uint32_t left)
{
    const uint32_t pw[4] = {pk.x, pk.y, pk.z, pk.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool valid = !kPartial || (uint32_t)j < left;
        const uint32_t pos = valid ? (pw[j >> 1] >> (16 * (j & 1))) & 0xFFFFu : 0u;
        if constexpr (NW == 2) {
            const uint2 v = reinterpret_cast<const uint2 *>(tabl)[pos];  // one ds_read_b64: the position's word pair
            x[0][j] = valid ? v.x : 0u;
            x[1][j] = valid ? v.y : 0u;
        } else {
            x[0][j] = valid ? tabl[pos] : 0u;
        }
    }
}

// Eight words into the ones, twos and fours of a counter set; the carry of weight eight is returned.
__device__ __forceinline__ uint32_t sp_tree8(uint32_t (&c)[kSpCounters], const uint32_t (&x)[8])
{
    uint32_t t0, t1, t2, t3, f0, f1, e;
    csa_sm(t0, c[0], c[0], x[0], x[1]);
    csa_sm(t1, c[0], c[0], x[2], x[3]);
    csa_sm(f0, c[1], c[1], t0, t1);
    csa_sm(t2, c[0], c[0], x[4], x[5]);
    csa_sm(t3, c[0], c[0], x[6], x[7]);
    csa_sm(f1, c[1], c[1], t2, t3);
    csa_sm(e, c[2], c[2], f0, f1);
    return e;
}

// a carry of weight 2^B ripples up the counter words
template <int B>
__device__ __forceinline__ void sp_ripple(uint32_t (&c)[kSpCounters], uint32_t e)
{
#pragma unroll
    for (int b = B; b < kSpCounters; ++b) {
        const uint32_t carry = c[b] & e;
        c[b] ^= e;
        e = carry;
    }
}

// A lane's walk: the groups of eight entries at k0, k0 + S, ... of the list lp[0 .. li).  Four whole steps at a time as a
// Harley-Seal tree over 32 entries -- the four carries of weight eight go through the eights and the sixteens, and ONE
// carry of weight 32 ripples into the upper words -- then what is left step by step, each one's eights rippled; only the
// list's last group can be partial.  Exact at every length: the counter words hold a set of up to 2047.
template <int NW, uint32_t S>
__device__ __forceinline__ void sp_walk(uint32_t (&c)[NW][kSpCounters], const uint32_t *tabl, const uint16_t *lp, uint32_t li, uint32_t k0)
{
    uint32_t x[NW][8];
    for (; k0 + 3 * S + 8 <= li; k0 += 4 * S) {
        uint32_t e[NW][4];
#pragma unroll
        for (uint32_t t = 0; t < 4; ++t) {
            sp_gather<NW, false>(x, tabl, *reinterpret_cast<const uint4 *>(lp + k0 + t * S), 8);
#pragma unroll
            for (int n = 0; n < NW; ++n) e[n][t] = sp_tree8(c[n], x[n]);
        }
#pragma unroll
        for (int n = 0; n < NW; ++n) {
            uint32_t sa, sb, th;
            csa_sm(sa, c[n][3], c[n][3], e[n][0], e[n][1]);
            csa_sm(sb, c[n][3], c[n][3], e[n][2], e[n][3]);
            csa_sm(th, c[n][4], c[n][4], sa, sb);
            sp_ripple<5>(c[n], th);
        }
    }
    for (; k0 + 8 <= li; k0 += S) {
        sp_gather<NW, false>(x, tabl, *reinterpret_cast<const uint4 *>(lp + k0), 8);
#pragma unroll
        for (int n = 0; n < NW; ++n) sp_ripple<3>(c[n], sp_tree8(c[n], x[n]));
    }
    if (k0 < li) {
        sp_gather<NW, true>(x, tabl, *reinterpret_cast<const uint4 *>(lp + k0), li - k0);
#pragma unroll
        for (int n = 0; n < NW; ++n) sp_ripple<3>(c[n], sp_tree8(c[n], x[n]));
    }
}

// a += the same counter words of the lane d away (a bit-sliced adder; every lane of the wave takes part)
__device__ __forceinline__ void sp_add_lane(uint32_t (&a)[kSpCounters], const uint32_t (&give)[kSpCounters], int d)
{
    uint32_t carry = 0;
#pragma unroll
    for (int b = 0; b < kSpCounters; ++b) {
        const uint32_t o = __shfl_xor(give[b], d, 64);
        const uint32_t u = a[b] ^ o;
        const uint32_t sum = u ^ carry;
        carry = (a[b] & o) | (u & carry);
        a[b] = sum;
    }
}

// The LDS placement, NW = 1 | 2 table words a workgroup (option sparse_words): 32 NW columns of the table slab, staged as
// [2^p positions][NW words] -- at NW = 2 a lane's ds_read_b64 returns the 64 column bits of a position for the LDS-array
// cycles a 32-bit read of one word takes, and the random positions of a wave's lanes conflict on the banks as often either
// way.  4 / NW workgroups per item, 512 NW lanes as (list row, 4 NW lanes of the row): lane q walks every (4 NW)th group of
// eight list entries into NW counter sets, the lanes of a row add their counters, and lane q reads out the columns
// 8 q .. 8 q + 7 of the 32 NW.  Workgroup g is (x, w, c) = (g % 8, (g / 8) % (4 / NW), g / 8 / (4 / NW)).  It takes the
// table words w NW .. and a RUN of `run` items of the launch, x + 8 * (c * run + i) for i < run: every eighth item, so that
// an item's launch position still names its XCD, and one behind the other there the planner puts items of one table block
// (plan.cpp, order_sparse_items).  The words are staged only where an item's table slab is not the one the item before it
// in the run left there (plan.h, sparse_table_fills counts by the same rule: four words per staging of an item's
// workgroups, at either NW); the set sizes lt of the lane's eight table columns stay in registers as long.
// lds: [2^p][NW] the table, then CT [32 NW][128]: the values of a transposed item on their way out, in a place of their
// own, so that the table outlives the item: 72 KiB at p = 14, NW = 1 and 16-bit C(v), 144 KiB at NW = 2.
// DSH_SPARSE_CUT (a measuring build, `make SPCUT=1`, never the product library): an item ends after phase `stop` -- 1 the
// fill, 2 the walk, 3 the lanes' addition -- and the results are meaningless; stop = 0 is the whole kernel.
template <typename CT, int NW>
__global__ __launch_bounds__(512 * NW) void k_sparse_count_lds(const uint4 *__restrict__ items, uint32_t nitems, uint32_t run,
                                                               const uint32_t *__restrict__ tabw, const uint16_t *__restrict__ lists,
                                                               const uint32_t *__restrict__ len, uint32_t cap, uint32_t m,
                                                               CT *__restrict__ cum, uint64_t nslots, uint32_t stop)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t sp_lds[];
#ifdef DSH_SPARSE_CUT
    const uint32_t cut = stop;
#else
    constexpr uint32_t cut = 0;
#endif
    constexpr uint32_t kThreads = 512 * NW, kLanes = 4 * NW, kGroups = 4 / NW, kCols = 32 * NW;  // lanes of a row; workgroups of an item; their columns
    CT *turn = reinterpret_cast<CT *>(sp_lds + (size_t)m * NW);
    const uint32_t g = blockIdx.x, x = g & 7u, w = (g >> 3) % kGroups, first = (g >> 3) / kGroups * run;
    const uint32_t tid = threadIdx.x, r = tid / kLanes, q = tid % kLanes, c0 = 8 * q;
    uint32_t have = 0xFFFFFFFFu;  // the table slab whose words the LDS holds
    uint32_t lt[8];
    // (every condition on the way to a barrier is uniform over the workgroup: the item, its slabs and its flags)
    for (uint32_t i = 0; i < run; ++i) {
        const uint32_t item = x + 8 * (first + i);
        if (item >= nitems) break;  // a ragged last run
        const uint4 it = items[item];
        const bool tr = (it.y & kSpItemTransposed) != 0;
        const uint32_t ls = tr ? it.w : it.z, ts = tr ? it.z : it.w, plane = it.y & kSpPlaneMask;  // list slab, table slab
        if (ts != have) {
            if (i) __syncthreads();  // the walk of the item before is over in every wave
            const uint4 *src = reinterpret_cast<const uint4 *>(tabw + ((uint64_t)ts * 4 + w * NW) * m);
            uint4 *dst = reinterpret_cast<uint4 *>(sp_lds);
            if constexpr (NW == 2) {  // the two word-major words, interleaved by position
                for (uint32_t k = tid; k < m / 4; k += kThreads) {
                    const uint4 a = src[k], b = src[m / 4 + k];
                    dst[2 * k] = make_uint4(a.x, b.x, a.y, b.y);
                    dst[2 * k + 1] = make_uint4(a.z, b.z, a.w, b.w);
                }
            } else {
                for (uint32_t k = tid; k < m / 4; k += kThreads) dst[k] = src[k];
            }
            const uint4 *lq = reinterpret_cast<const uint4 *>(len + (uint64_t)ts * kTile + w * kCols + c0);
            const uint4 l0 = lq[0], l1 = lq[1];
            lt[0] = l0.x, lt[1] = l0.y, lt[2] = l0.z, lt[3] = l0.w, lt[4] = l1.x, lt[5] = l1.y, lt[6] = l1.z, lt[7] = l1.w;
            __syncthreads();
            have = ts;
        }
        if (cut == 1) continue;
        const uint32_t li_all = len[(uint64_t)ls * kTile + r];
        const uint32_t li = li_all < cap ? li_all : cap;
        uint32_t c[NW][kSpCounters];
#pragma unroll
        for (int n = 0; n < NW; ++n)
#pragma unroll
            for (int b = 0; b < kSpCounters; ++b) c[n][b] = 0;
        sp_walk<NW, 8 * kLanes>(c, sp_lds, lists + ((uint64_t)ls * kTile + r) * cap, li, c0);
        if (cut == 2) continue;
        // The lanes of a row add their counters.  At NW = 2 the lanes 4 apart first swap halves: a lane gives away the set
        // it will not read out and keeps the row's sum of the other; then, as at NW = 1, the four lanes of that half.
        uint32_t s[kSpCounters];
#pragma unroll
        for (int b = 0; b < kSpCounters; ++b) s[b] = NW == 2 && (q & 4u) ? c[NW - 1][b] : c[0][b];
        if constexpr (NW == 2) {
            uint32_t give[kSpCounters];
#pragma unroll
            for (int b = 0; b < kSpCounters; ++b) give[b] = q & 4u ? c[0][b] : c[1][b];
            sp_add_lane(s, give, 4);
        }
        sp_add_lane(s, s, 1);
        sp_add_lane(s, s, 2);
        if (cut == 3) {  // (the sum leaves the lane, so that the phase is not compiled away; no value of a real item is all ones)
            uint32_t all = 0xFFFFFFFFu;
#pragma unroll
            for (int b = 0; b < kSpCounters; ++b) all &= s[b];
            if (all == 0xFFFFFFFFu && cap == 1) turn[tid] = (CT)all;
            continue;
        }
        // every lane of a row now holds the row's counters of its word: lane q reads out 8 of the 32 NW columns
        uint32_t out[8];
        sp_values<CT, 8>(out, s, c0 & 31u, it.y, m, li_all, lt);
        CT *blk = cum + (uint64_t)plane * nslots + (uint64_t)it.x * (kTile * kTile);
        if (!tr) {  // a row's lanes store 32 NW values side by side
            put8(blk + (uint64_t)r * kTile + w * kCols + c0, out);
            continue;
        }
        // transposed: lane (r, q) holds column r of the rows w * 32 NW + 8 q .. + 7.  The 32 NW x 128 values are turned in
        // LDS and leave as whole rows, which lie one behind the other in the tile's block.  The first barrier: the rows of
        // a transposed item before this one have left
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 8; ++j) turn[(c0 + j) * kTile + r] = (CT)out[j];
        __syncthreads();
        const uint4 *ts4 = reinterpret_cast<const uint4 *>(turn);
        uint4 *dst = reinterpret_cast<uint4 *>(blk + (uint64_t)w * kCols * kTile);
        for (uint32_t k = tid; k < kCols * kTile * sizeof(CT) / 16; k += kThreads) dst[k] = ts4[k];
    }
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

namespace {

// NW words of the table and the turned values of a transposed item: at p = 14 and 16-bit C(v) 72 KiB (NW = 1: two
// workgroups of 512 lanes a CU) or 144 KiB (NW = 2: one of 1 024)
template <typename CT, int NW>
hipError_t launch_sparse_count_lds(hipStream_t st, uint32_t runs, const uint4 *items, uint32_t nitems, uint32_t run, const uint32_t *tab,
                                   const uint16_t *lists, const uint32_t *len, uint32_t cap, uint32_t m, void *cum, uint64_t nslots)
{
    const size_t lds = ((size_t)m * 4 + 32 * kTile * sizeof(CT)) * NW;
    if (lds > 160 * 1024) return hipErrorInvalidValue;  // (the NW words of the table in a CU's LDS)
    const hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(k_sparse_count_lds<CT, NW>), lds);
    if (e != hipSuccess) return e;
    uint32_t stop = 0;
#ifdef DSH_SPARSE_CUT
    if (const char *s = std::getenv("DSH_SPARSE_STOP")) stop = (uint32_t)std::atoi(s);
#endif
    hipLaunchKernelGGL((k_sparse_count_lds<CT, NW>), dim3(runs * 8 * (4 / NW)), dim3(512 * NW), lds, st, items, nitems, run, tab, lists, len,
                       cap, m, (CT *)cum, nslots, stop);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_sparse_count(hipStream_t st, int cum_bytes, const uint4 *items, uint32_t nitems, uint32_t run, int wordmajor, int words,
                               const uint32_t *tab, const uint16_t *lists, const uint32_t *len, uint32_t cap, uint32_t m, void *cum,
                               uint64_t nslots)
{
    if (nitems == 0) return hipSuccess;
    if (cap % 8 || cap > 2047 || run == 0) return hipErrorInvalidValue;
    if (wordmajor) {
        if (m < 512 || m > (1u << 15) || (words != 1 && words != 2)) return hipErrorInvalidValue;
        const uint32_t per_x = (nitems + 7) / 8;  // the items of an XCD residue
        run = std::min(run, per_x);
        const uint32_t runs = (per_x + run - 1) / run;
        if (words == 2) {  // (16-bit C(v) only: it is 32 bits wide at p = 16, where the table is gathered)
            if (cum_bytes != 2) return hipErrorInvalidValue;
            return launch_sparse_count_lds<uint16_t, 2>(st, runs, items, nitems, run, tab, lists, len, cap, m, cum, nslots);
        }
        return cum_bytes == 2 ? launch_sparse_count_lds<uint16_t, 1>(st, runs, items, nitems, run, tab, lists, len, cap, m, cum, nslots)
                              : launch_sparse_count_lds<uint32_t, 1>(st, runs, items, nitems, run, tab, lists, len, cap, m, cum, nslots);
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
