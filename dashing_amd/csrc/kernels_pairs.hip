// kernels_pairs.hip -- the DIRECT form of a comparison, for an explicit list of pairs (dsh_dist_pairs*, pairs.hip,
// DESIGN.md 4.8): read the two register rows, take the exact histogram of max(a, b), run the estimator -- what
// k_selfhist_card + k_card_from_hist do for a sketch, done for a pair, with the estimators of estimators.h as they are.
// The bit-plane tile machinery (kernels_compare.hip) is not involved: its unit is a 128 x 128 tile of a key-ordered
// layout, a sparse list wants 2 * 2^p bytes per pair and nothing else.
//
//   k_pairs_hist    one wave per pair: 64-bin histogram of max(a, b) (LDS atomics on privatised sub-histograms), the
//                   out-of-range test on the loaded words.  With lhs == nullptr the "pairs" are (s, s), s = first ...:
//                   max(a, a) = a, the sketches' own histograms (the cardinality pass).
//   k_pairs_card    one lane per sketch: cardinality from its own histogram (k_card_from_hist's job, own buffer)
//   k_pairs_finish  one lane per pair: union size from the pair's histogram, the two cardinalities, every requested measure
// Histograms travel between the kernels as 64 counters per pair, uint16 up to p = 15 (a bin holds at most 2^p).
#include "estimators.h"
#include "kernels.h"

namespace dsh {

namespace {

// byte-wise max of two words of register bytes (all < 128: the borrow of a byte never reaches its neighbour, as in
// k_selfhist_card's `hits`).  Out-of-range bytes give garbage here; the call that saw them fails.
__device__ __forceinline__ uint32_t max_u8x4(uint32_t a, uint32_t b)
{
    const uint32_t ge = ((a | 0x80808080u) - b) & 0x80808080u;  // bit 7 of byte k: a_k >= b_k
    const uint32_t mask = (ge >> 7) * 0xFFu;
    return (a & mask) | (b & ~mask);
}

// bit 7 of byte k set iff byte k is >= 128 or >= q + 2 (limrep = (q + 2) in every byte): k_selfhist_card's test
__device__ __forceinline__ uint32_t bad_u8x4(uint32_t w, uint32_t limrep)
{
    return (w | (((w & 0x7F7F7F7Fu) | 0x80808080u) - limrep)) & 0x80808080u;
}

}  // namespace

// err[0]: smallest list index of a pair that names a slot >= n; err[1]: smallest sketch named by a pair that holds an
// out-of-range register (both start at ~0).  err == nullptr (the cardinality pass): a sketch with such a register gets
// the histogram of an empty sketch instead -- nothing is reported for sketches no pair names.
template <typename CT>
__global__ __launch_bounds__(256, 4) void k_pairs_hist(const uint8_t *__restrict__ regs, uint64_t n, int p,
                                                      const uint32_t *__restrict__ lhs, const uint32_t *__restrict__ rhs,
                                                      uint64_t first, uint64_t xbase, uint64_t cnt, CT *__restrict__ hist_out,
                                                      unsigned long long *__restrict__ err)
{
    __shared__ uint32_t sub[4][8][72];  // 8 privatised, bank-spread copies per wave: see k_selfhist_card
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t xi = (uint64_t)blockIdx.x * 4 + wave;  // pairs [0, cnt) of this launch
#pragma unroll
    for (int k = 0; k < 8; ++k) sub[wave][k][lane] = 0;
    __syncthreads();
    bool live = xi < cnt;
    uint64_t sa = 0, sb = 0;
    if (live) {
        sa = lhs ? (uint64_t)lhs[xi] : first + xi;
        sb = lhs ? (uint64_t)rhs[xi] : first + xi;
        if (sa >= n || sb >= n) {
            if (lane == 0 && err) atomicMin(&err[0], (unsigned long long)(xbase + xi));
            live = false;
        }
    }
    const uint64_t m = 1ull << p;
    const uint64_t nch = m >> 4;  // 16-byte chunks of a row
    uint32_t bada = 0, badb = 0;
    if (live) {
        const uint4 *__restrict__ ra = reinterpret_cast<const uint4 *>(regs + sa * m);
        const uint4 *__restrict__ rb = reinterpret_cast<const uint4 *>(regs + sb * m);
        const uint32_t limrep = (uint32_t)(64 - p + 2) * 0x01010101u;
        uint32_t *mysub = sub[wave][lane & 7];
        auto count16 = [mysub, limrep, &bada, &badb](const uint4 a, const uint4 b) {
            const uint32_t wa[4] = {a.x, a.y, a.z, a.w}, wb[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                bada |= bad_u8x4(wa[k], limrep);
                badb |= bad_u8x4(wb[k], limrep);
                const uint32_t w = max_u8x4(wa[k], wb[k]);
                atomicAdd(&mysub[w & 63], 1u);
                atomicAdd(&mysub[(w >> 8) & 63], 1u);
                atomicAdd(&mysub[(w >> 16) & 63], 1u);
                atomicAdd(&mysub[(w >> 24) & 63], 1u);
            }
        };
        // whole rounds of kU chunks per lane with every load of both rows in flight together, then the rest one at a time
        // (p <= 11: the rest is all there is, at most two chunks per lane)
        constexpr int kU = 4;  // (kU and the launch bounds are first choices, not the winners of an A/B: DESIGN.md 4.8, Not measured)
        const uint64_t nfull = nch / (kU * 64) * (kU * 64);  // chunks in whole rounds
        uint64_t c = lane;
        for (; c < nfull; c += (uint64_t)kU * 64) {
            uint4 a[kU], b[kU];
#pragma unroll
            for (int k = 0; k < kU; ++k) a[k] = ra[c + (uint64_t)k * 64];
#pragma unroll
            for (int k = 0; k < kU; ++k) b[k] = rb[c + (uint64_t)k * 64];
#pragma unroll
            for (int k = 0; k < kU; ++k) count16(a[k], b[k]);
        }
        for (; c < nch; c += 64) count16(ra[c], rb[c]);
    }
    __syncthreads();
    if (!live) return;
    uint32_t t = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) t += sub[wave][k][lane];
    const bool anya = __ballot(bada != 0) != 0, anyb = __ballot(badb != 0) != 0;
    if (anya || anyb) {
        if (err) {
            if (lane == 0) atomicMin(&err[1], (unsigned long long)(anya && anyb ? (sa < sb ? sa : sb) : anya ? sa : sb));
        } else {
            t = 0;  // with CT = uint16_t m is at most 2^15
            if (lane == 0) t = (uint32_t)m;
        }
    }
    hist_out[xi * 64 + lane] = (CT)t;
}

namespace {

// The histograms of the 64 pairs (sketches) [blk * 64, ...) of a launch, one LDS column per lane: bin v of lane l is
// col[v * STRIDE + l], conflict-free for the estimator's reads; STRIDE is odd in 32-bit words (66 uint16 = 33 words, 65
// uint32) so the transposing writes spread over the banks too.
template <typename CT>
struct ColStride {
    enum { value = sizeof(CT) == 2 ? 66 : 65 };
};

template <typename CT>
__device__ __forceinline__ void load_cols(const CT *__restrict__ hist, uint64_t x0, uint64_t cnt, CT *col)
{
    constexpr int S = ColStride<CT>::value;
    const int lane = threadIdx.x;
#pragma unroll 8
    for (int k = 0; k < 64; ++k)  // pair k of the block, bin = lane: one coalesced row per step
        col[lane * S + k] = x0 + k < cnt ? hist[(x0 + k) * 64 + lane] : (CT)0;
    __syncthreads();
}

template <typename CT>
struct Col {  // bin v of this lane's histogram, and its address (estimators.h: Hist and Raw)
    const CT *col;
    enum { stride = ColStride<CT>::value };
    __device__ uint32_t operator()(int v) const { return col[(v & 63) * stride]; }
    __device__ const CT *at(int v) const { return col + v * stride; }  // (v - 1 >= 0 wherever the estimator reads ahead)
};

// estimate() on this lane's column, the hints being the exact live range
template <typename CT>
__device__ __forceinline__ double estimate_col(const CT *mycol, int p, int estim)
{
    const Col<CT> c{mycol};
    int lo = 0, hi = 63;
    while (lo < 63 && c(lo) == 0) ++lo;
    while (hi > lo && c(hi) == 0) --hi;
    return estimate(c, c, p, estim, lo, hi);
}

}  // namespace

template <typename CT>
__global__ __launch_bounds__(64) void k_pairs_card(const CT *__restrict__ hist, uint64_t first, uint64_t cnt, int p, int estim,
                                                   double *__restrict__ card)
{
    __shared__ CT col[64 * ColStride<CT>::value];
    const uint64_t x0 = (uint64_t)blockIdx.x * 64, xi = x0 + threadIdx.x;
    load_cols(hist, x0, cnt, col);
    if (xi >= cnt) return;
    card[first + xi] = estimate_col(col + threadIdx.x, p, estim);
}

template <typename CT>
__global__ __launch_bounds__(64) void k_pairs_finish(const CT *__restrict__ hist, const uint32_t *__restrict__ lhs,
                                                     const uint32_t *__restrict__ rhs, uint64_t n, uint64_t cnt, int p, int estim,
                                                     const double *__restrict__ card, PairsTypes types, uint32_t n_types,
                                                     double ksinv, float *__restrict__ out, uint64_t out_stride)
{
    __shared__ CT col[64 * ColStride<CT>::value];
    const uint64_t x0 = (uint64_t)blockIdx.x * 64, xi = x0 + threadIdx.x;
    load_cols(hist, x0, cnt, col);
    if (xi >= cnt) return;
    const uint64_t sa = lhs[xi], sb = rhs[xi];
    if (sa >= n || sb >= n) return;  // (reported by k_pairs_hist: the call fails)
    const double mys = card[sa], os = card[sb];
    const double us = estimate_col(col + threadIdx.x, p, estim);
    for (uint32_t t = 0; t < n_types; ++t) out[(uint64_t)t * out_stride + xi] = result_cmp_from(mys, os, us, types.t[t], ksinv);
}

hipError_t launch_pairs_hist(hipStream_t st, const uint8_t *regs, uint64_t n, int p, const uint32_t *lhs, const uint32_t *rhs,
                             uint64_t first, uint64_t xbase, uint64_t cnt, void *hist, unsigned long long *err)
{
    if (!cnt) return hipSuccess;
    const dim3 grid((uint32_t)((cnt + 3) / 4));
    if (p <= kPairsMaxP16)
        hipLaunchKernelGGL(k_pairs_hist<uint16_t>, grid, dim3(256), 0, st, regs, n, p, lhs, rhs, first, xbase, cnt, (uint16_t *)hist, err);
    else
        hipLaunchKernelGGL(k_pairs_hist<uint32_t>, grid, dim3(256), 0, st, regs, n, p, lhs, rhs, first, xbase, cnt, (uint32_t *)hist, err);
    return hipGetLastError();
}

hipError_t launch_pairs_card(hipStream_t st, const void *hist, uint64_t first, uint64_t cnt, int p, int estim, double *card)
{
    if (!cnt) return hipSuccess;
    const dim3 grid((uint32_t)((cnt + 63) / 64));
    if (p <= kPairsMaxP16)
        hipLaunchKernelGGL(k_pairs_card<uint16_t>, grid, dim3(64), 0, st, (const uint16_t *)hist, first, cnt, p, estim, card);
    else
        hipLaunchKernelGGL(k_pairs_card<uint32_t>, grid, dim3(64), 0, st, (const uint32_t *)hist, first, cnt, p, estim, card);
    return hipGetLastError();
}

hipError_t launch_pairs_finish(hipStream_t st, const void *hist, const uint32_t *lhs, const uint32_t *rhs, uint64_t n, uint64_t cnt,
                               int p, int estim, const double *card, const PairsTypes &types, uint32_t n_types, double ksinv,
                               float *out, uint64_t out_stride)
{
    if (!cnt || !n_types) return hipSuccess;
    const dim3 grid((uint32_t)((cnt + 63) / 64));
    if (p <= kPairsMaxP16)
        hipLaunchKernelGGL(k_pairs_finish<uint16_t>, grid, dim3(64), 0, st, (const uint16_t *)hist, lhs, rhs, n, cnt, p, estim, card,
                           types, n_types, ksinv, out, out_stride);
    else
        hipLaunchKernelGGL(k_pairs_finish<uint32_t>, grid, dim3(64), 0, st, (const uint32_t *)hist, lhs, rhs, n, cnt, p, estim, card,
                           types, n_types, ksinv, out, out_stride);
    return hipGetLastError();
}

}  // namespace dsh
