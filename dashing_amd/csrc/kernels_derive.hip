// kernels_derive.hip -- new sketches out of resident ones (dsh_fold*, dsh_upload_sketches_folded*, dsh_union_groups*,
// derive.hip): dashing's hll_t::compress (fold to a lower precision) and hll_t::operator+= (register-wise
// maximum).  Both are pure streaming over register rows: every source byte is read once, far fewer are written.
//
//   k_fold          rows [n][2^ps] -> rows [n][2^pd], d = ps - pd.  Rows lie back to back on both sides, so the job is
//                   flat: output byte J is the fold of the RUN of 2^d source bytes [J << d, (J + 1) << d).  With
//                   low = index inside the run, a non-empty register contributes v + d at low == 0 and
//                   clz_d(low) + 1 = d - msb(low) elsewhere.  msb is monotone, so of the registers behind the first only
//                   the first non-empty one matters, and v + d >= d + 1 beats them all:
//                       out = v0 ? v0 + d : (first non-empty low exists ? d - msb(low) : 0)
//                   Every contribution is computed with the full d, so partial results combine with a plain max:
//                   inside a lane (16 bytes, d <= 4), across the lanes of a wave (1 KiB, d <= 10), across waves and
//                   passes of a workgroup through LDS (above).
//   k_union_groups  out[v] = byte-wise max of the rows a CSR names; one lane owns 16 bytes of one output row.
#include "kernels.h"

namespace dsh {

namespace {

constexpr int kFoldThreads = 256;
constexpr int kFoldUnroll = 4;                                   // 16-byte loads a lane has in flight
constexpr uint32_t kFoldStepLog = 14;                            // bytes a workgroup takes per step: 256 x 16 x 4

template <bool AL>
__device__ __forceinline__ uint4 load16(const uint8_t *p)
{
    if (AL) return *(const uint4 *)p;
    uint32_t w[4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        w[k] = (uint32_t)p[4 * k] | (uint32_t)p[4 * k + 1] << 8 | (uint32_t)p[4 * k + 2] << 16 | (uint32_t)p[4 * k + 3] << 24;
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// bit 7 of byte k: byte k of w is above the cap (add = (127 - cap) in every byte, cap < 127)
__device__ __forceinline__ uint32_t over_u8x4(uint32_t w, uint32_t add) { return (((w & 0x7F7F7F7Fu) + add) | w) & 0x80808080u; }

// the fold of one run of 2^d <= 8 bytes, held in the low bytes of x (the rest zero)
__device__ __forceinline__ uint32_t fold_run(uint64_t x, int d)
{
    const uint32_t b0 = (uint32_t)x & 0xFFu;
    if (b0) return b0 + d;
    x >>= 8;
    if (!x) return 0;
    const uint32_t f = ((uint32_t)(__ffsll((unsigned long long)x) - 1) >> 3) + 1;  // index of the first non-empty register
    return (uint32_t)d - (31 - __clz((int)f));
}

// what the 16 bytes of chunk number c of a run contribute (d >= 4; c = 0: the chunk that holds low == 0)
__device__ __forceinline__ uint32_t fold_chunk(uint4 v, uint32_t c, int d)
{
    const uint64_t lo = v.x | (uint64_t)v.y << 32, hi = v.z | (uint64_t)v.w << 32;
    if (!(lo | hi)) return 0;
    if (c) return (uint32_t)d - 4 - (31 - __clz((int)c));  // low = 16 c + f: msb(low) = 4 + msb(c) whatever f is
    const uint32_t b0 = (uint32_t)lo & 0xFFu;
    if (b0) return b0 + d;
    const uint64_t r = lo >> 8;
    const uint32_t f = r ? ((uint32_t)(__ffsll((unsigned long long)r) - 1) >> 3) + 1 : 8 + ((uint32_t)(__ffsll((unsigned long long)hi) - 1) >> 3);
    return (uint32_t)d - (31 - __clz((int)f));
}

// A workgroup owns a TILE of 2^tlog source bytes: 16 KiB (one step) up to d = 10, above that the 16 runs that make 16
// output bytes (2^(d - 10) steps).  Its output bytes are collected in LDS and stored once.  total = n << ps source bytes
// (a multiple of the run, and of the tile where d > 10); err: smallest row0 + row that holds a register above the cap.
template <bool SRC_AL, bool DST_AL>
__global__ __launch_bounds__(kFoldThreads) void k_fold(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, uint64_t total,
                                                       int ps, int d, uint64_t row0, unsigned long long *__restrict__ err)
{
    __shared__ __attribute__((aligned(16))) uint8_t sm[1u << kFoldStepLog];
    uint32_t *smw = (uint32_t *)sm;
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t tlog = d <= 10 ? kFoldStepLog : (uint32_t)d + 4;
    const uint64_t t0 = (uint64_t)blockIdx.x << tlog;
    const uint32_t nsteps = 1u << (tlog - kFoldStepLog);
    const uint32_t capadd = (uint32_t)(127 - (64 - ps + 1)) * 0x01010101u;
    const uint32_t cmask = d > 4 ? (1u << (d - 4)) - 1 : 0;       // chunk number inside a run
    const uint32_t group = d > 4 ? (d < 10 ? 1u << (d - 4) : 64u) : 1u;  // lanes that share a run
    if (d > 10) {
        if (tid < 16) smw[tid] = 0;
        __syncthreads();
    }
    for (uint32_t s = 0; s < nsteps; ++s) {
        uint4 v[kFoldUnroll];
        uint64_t off[kFoldUnroll];
#pragma unroll
        for (int u = 0; u < kFoldUnroll; ++u) {
            off[u] = t0 + ((uint64_t)s << kFoldStepLog) + (uint32_t)u * (kFoldThreads * 16) + tid * 16;
            v[u] = off[u] < total ? load16<SRC_AL>(src + off[u]) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int u = 0; u < kFoldUnroll; ++u) {
            if (over_u8x4(v[u].x, capadd) | over_u8x4(v[u].y, capadd) | over_u8x4(v[u].z, capadd) | over_u8x4(v[u].w, capadd))
                atomicMin(err, (unsigned long long)(row0 + (off[u] >> ps)));
            const uint32_t in_tile = (uint32_t)u * (kFoldThreads * 16) + tid * 16;  // (d <= 10: one step, offset in the tile)
            if (d >= 4) {
                uint32_t val = fold_chunk(v[u], (uint32_t)(off[u] >> 4) & cmask, d);
                for (uint32_t m = 1; m < group; m <<= 1) val = max(val, (uint32_t)__shfl_xor((int)val, (int)m));
                if (d <= 10) {
                    if (!(lane & (group - 1))) sm[in_tile >> d] = (uint8_t)val;
                } else if (lane == 0) {
                    atomicMax(&smw[(uint32_t)((off[u] - t0) >> d)], val);
                }
            } else if (d == 0) {
                *(uint4 *)(sm + in_tile) = v[u];
            } else if (d == 1) {
                const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
                uint32_t o[2] = {0, 0};
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i >> 2] |= fold_run((w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu, 1) << (8 * (i & 3));
                *(uint2 *)(sm + (in_tile >> 1)) = make_uint2(o[0], o[1]);
            } else if (d == 2) {
                *(uint32_t *)(sm + (in_tile >> 2)) = fold_run(v[u].x, 2) | fold_run(v[u].y, 2) << 8 | fold_run(v[u].z, 2) << 16 | fold_run(v[u].w, 2) << 24;
            } else {
                *(uint16_t *)(sm + (in_tile >> 3)) =
                    (uint16_t)(fold_run(v[u].x | (uint64_t)v[u].y << 32, 3) | fold_run(v[u].z | (uint64_t)v[u].w << 32, 3) << 8);
            }
        }
    }
    __syncthreads();
    uint8_t *ob = dst + (t0 >> d);
    if (d <= 10) {
        const uint64_t left = total - t0;
        const uint32_t nout = (uint32_t)(left < (1u << kFoldStepLog) ? left : (1u << kFoldStepLog)) >> d;  // a multiple of 16
        if (DST_AL) {
            for (uint32_t i = tid * 16; i < nout; i += kFoldThreads * 16) *(uint4 *)(ob + i) = *(const uint4 *)(sm + i);
        } else {
            for (uint32_t i = tid; i < nout; i += kFoldThreads) ob[i] = sm[i];
        }
    } else if (DST_AL) {
        if (tid < 4) *(uint32_t *)(ob + 4 * tid) = smw[4 * tid] | smw[4 * tid + 1] << 8 | smw[4 * tid + 2] << 16 | smw[4 * tid + 3] << 24;
    } else if (tid < 16) {
        ob[tid] = (uint8_t)smw[tid];
    }
}

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

// byte-wise max kept as two words of 16-bit halves (even bytes, odd bytes): any byte values, two packed max per word
struct MaxAcc {
    us2 e[4], o[4];
    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int k = 0; k < 4; ++k) e[k] = o[k] = (us2)(0);
    }
    __device__ __forceinline__ void add(uint4 v)
    {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t we = w[k] & 0x00FF00FFu, wo = (w[k] >> 8) & 0x00FF00FFu;
            e[k] = __builtin_elementwise_max(e[k], __builtin_bit_cast(us2, we));
            o[k] = __builtin_elementwise_max(o[k], __builtin_bit_cast(us2, wo));
        }
    }
    __device__ __forceinline__ uint32_t word(int k) const { return __builtin_bit_cast(uint32_t, e[k]) | __builtin_bit_cast(uint32_t, o[k]) << 8; }
};

// Lane q of the launch owns bytes [16 q, 16 q + 16) of the flat output [nv][2^p]: row v = 16 q >> p.  Its members are
// mem[ptr[v] .. ptr[v + 1]) (mem == nullptr: the rows ptr[v] .. ptr[v + 1) themselves) of `src`; the row goes to
// out_a + dst[v] * 2^p, or, with bit 31 of dst[v] set, to out_b + (dst[v] & 0x7FFFFFFF) * 2^p (dst == nullptr: out_a, row v).
// Only out_a may be misaligned (DST_AL = false: byte stores there).
template <bool DST_AL>
__global__ __launch_bounds__(256) void k_union_groups(const uint8_t *__restrict__ src, int p, const uint64_t *__restrict__ ptr,
                                                      const uint32_t *__restrict__ mem, const uint32_t *__restrict__ dst, uint64_t nv,
                                                      uint8_t *__restrict__ out_a, uint8_t *__restrict__ out_b)
{
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t v = (q << 4) >> p;
    if (v >= nv) return;
    const uint64_t off = (q << 4) & (((uint64_t)1 << p) - 1);
    const uint64_t b = ptr[v], e = ptr[v + 1];
    MaxAcc acc;
    acc.zero();
    uint64_t x = b;
    for (; x + 4 <= e; x += 4) {
        uint4 r[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) r[u] = *(const uint4 *)(src + ((uint64_t)(mem ? mem[x + u] : x + u) << p) + off);
#pragma unroll
        for (int u = 0; u < 4; ++u) acc.add(r[u]);
    }
    for (; x < e; ++x) acc.add(*(const uint4 *)(src + ((uint64_t)(mem ? mem[x] : x) << p) + off));
    const uint32_t dv = dst ? dst[v] : (uint32_t)v;
    if (dv & 0x80000000u) {
        *(uint4 *)(out_b + ((uint64_t)(dv & 0x7FFFFFFFu) << p) + off) = make_uint4(acc.word(0), acc.word(1), acc.word(2), acc.word(3));
        return;
    }
    uint8_t *o = out_a + ((uint64_t)dv << p) + off;
    if (DST_AL) {
        *(uint4 *)o = make_uint4(acc.word(0), acc.word(1), acc.word(2), acc.word(3));
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t w = acc.word(k);
            o[4 * k] = (uint8_t)w, o[4 * k + 1] = (uint8_t)(w >> 8), o[4 * k + 2] = (uint8_t)(w >> 16), o[4 * k + 3] = (uint8_t)(w >> 24);
        }
    }
}

}  // namespace

hipError_t launch_fold(hipStream_t st, const uint8_t *src, uint64_t n, int ps, int pd, uint64_t row0, uint8_t *dst,
                       unsigned long long *err)
{
    if (!n) return hipSuccess;
    const int d = ps - pd;
    const uint64_t total = n << ps;
    const uint32_t tlog = d <= 10 ? kFoldStepLog : (uint32_t)d + 4;
    const uint64_t blocks = (total + (((uint64_t)1 << tlog) - 1)) >> tlog;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const bool sa = !((uintptr_t)src & 15), da = !((uintptr_t)dst & 15);
    auto k = sa ? (da ? k_fold<true, true> : k_fold<true, false>) : (da ? k_fold<false, true> : k_fold<false, false>);
    hipLaunchKernelGGL(k, dim3((uint32_t)blocks), dim3(kFoldThreads), 0, st, src, dst, total, ps, d, row0, err);
    return hipGetLastError();
}

hipError_t launch_union_groups(hipStream_t st, const uint8_t *src, int p, const uint64_t *ptr, const uint32_t *mem,
                               const uint32_t *dst, uint64_t nv, uint8_t *out_a, uint8_t *out_b)
{
    if (!nv) return hipSuccess;
    const uint64_t lanes = (nv << p) >> 4, blocks = (lanes + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if ((uintptr_t)out_a & 15)
        hipLaunchKernelGGL(k_union_groups<false>, dim3((uint32_t)blocks), dim3(256), 0, st, src, p, ptr, mem, dst, nv, out_a, out_b);
    else
        hipLaunchKernelGGL(k_union_groups<true>, dim3((uint32_t)blocks), dim3(256), 0, st, src, p, ptr, mem, dst, nv, out_a, out_b);
    return hipGetLastError();
}

}  // namespace dsh
