// kernels_curve.hip -- union growth curves (dsh_union_curve*, curve.hip): for every prefix of an order of
// resident sketches the register histogram of the prefix's union, from which launch_pairs_card (kernels_pairs.hip) takes
// the cardinality.  The union's registers are the running byte-wise maximum along the order; a register changes about
// ln(len) times, so the per-prefix histograms are not recounted: they are the prefix sums of the sparse stream of
// "a register moved from bin a to bin b at step i" events.
//
//   k_curve_walk    streams the rows of an (order, segment) once; a lane owns 16 registers and keeps their running
//                   maximum; what a step changes goes as -1 / +1 into delta[order][step][64] (int32, zeroed per batch)
//   k_curve_starts  with more than one segment per order: the segments' unions (launch_union_groups) turned into the
//                   exclusive running maxima the walk starts from, in place
//   k_curve_scan*   hist[o][i][v] = base[v] + sum over j <= i of delta[o][j][v], base = all 2^p registers in bin 0: chunk
//                   sums, their exclusive scan per order, then every chunk from its offset -- into the counters
//                   launch_pairs_card reads and, when asked, the caller's uint32 histogram
// All sums are integers: the result depends on no launch geometry, segment length or order of arrival of the atomics.
// Every loop is bounded by len; no workgroup waits for another.
#include "kernels.h"

namespace dsh {

namespace {

constexpr int kCurveLoads = kCurveLoadsInFlight;  // rows whose 16-byte loads a lane has in flight (a first choice, as k_union_groups')
constexpr uint32_t kScanChunk = kCurveScanChunk;
constexpr int kScanLoads = 8;                      // independent loads a scan lane has in flight

// byte-wise max of two words of register bytes, all < 128 (kernels_pairs.hip has the derivation); out-of-range bytes
// give garbage, and the call that saw them fails
__device__ __forceinline__ uint32_t max_u8x4(uint32_t a, uint32_t b)
{
    const uint32_t ge = ((a | 0x80808080u) - b) & 0x80808080u;
    const uint32_t mask = (ge >> 7) * 0xFFu;
    return (a & mask) | (b & ~mask);
}

// bit 7 of byte k set iff byte k is >= 128 or >= q + 2 (limrep = (q + 2) in every byte): k_pairs_hist's test
__device__ __forceinline__ uint32_t bad_u8x4(uint32_t w, uint32_t limrep)
{
    return (w | (((w & 0x7F7F7F7Fu) | 0x80808080u) - limrep)) & 0x80808080u;
}

// Lane q of the launch owns bytes [16 q, 16 q + 16) of the flat [nunits][2^p]: unit u = 16 q >> p is segment s = u % nseg of
// order o = u / nseg of the batch, its members ord[o * len + j], j in [s * S, min((s + 1) * S, len)).  cur starts as row u of
// `start` (s > 0) or zero.  WAVE_UNIT (p >= 10): a wave lies inside one unit, so the members and the rows' addresses are
// wave-uniform and the wave collects a step's moves in its own 64 bins of LDS -- wave-private, no workgroup barrier --
// before lane v adds bin v to delta.  Below p = 10 a wave holds several units: every changed byte goes to delta directly.
// A member >= n is skipped (the entry points have refused it).  err: smallest member that holds an out-of-range register.
template <bool WAVE_UNIT>
__global__ __launch_bounds__(256) void k_curve_walk(const uint8_t *__restrict__ regs, uint64_t n, int p,
                                                    const uint32_t *__restrict__ ord, uint64_t len, uint64_t S, uint32_t nseg,
                                                    uint32_t nunits, const uint8_t *__restrict__ start, int *__restrict__ delta,
                                                    unsigned long long *__restrict__ err)
{
    __shared__ int bins[4][64];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t uu = (q << 4) >> p;
    uint32_t u = uu < nunits ? (uint32_t)uu : nunits;
    if (WAVE_UNIT) u = (uint32_t)__builtin_amdgcn_readfirstlane((int)u);
    const bool live = u < nunits;
    if (WAVE_UNIT && !live) return;
    const uint64_t off = (q << 4) & (((uint64_t)1 << p) - 1);
    const uint32_t o = live ? u / nseg : 0, s = live ? u - o * nseg : 0;
    const uint64_t b = (uint64_t)s * S, e = live ? (b + S < len ? b + S : len) : 0;
    const uint32_t *__restrict__ ov = ord + (uint64_t)o * len;
    int *__restrict__ dl = delta + (((uint64_t)o * len) << 6);
    uint32_t cur[4] = {0, 0, 0, 0};
    if (live && s) {
        const uint4 c0 = *(const uint4 *)(start + ((uint64_t)u << p) + off);
        cur[0] = c0.x, cur[1] = c0.y, cur[2] = c0.z, cur[3] = c0.w;
    }
    const uint32_t limrep = (uint32_t)(64 - p + 2) * 0x01010101u;
    if (WAVE_UNIT) bins[wave][lane] = 0;
    for (uint64_t j = b; j < e; j += kCurveLoads) {
        uint32_t idx[kCurveLoads];
        uint4 r[kCurveLoads];
#pragma unroll
        for (int k = 0; k < kCurveLoads; ++k) idx[k] = j + k < e ? ov[j + k] : 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < kCurveLoads; ++k)
            r[k] = idx[k] < n ? *(const uint4 *)(regs + ((uint64_t)idx[k] << p) + off) : make_uint4(0, 0, 0, 0);
#pragma unroll
        for (int k = 0; k < kCurveLoads; ++k) {
            // (a member that was not loaded is a row of zeros: it changes nothing)
            const uint32_t w[4] = {r[k].x, r[k].y, r[k].z, r[k].w};
            uint32_t nw[4], chg = 0, bad = 0;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                bad |= bad_u8x4(w[t], limrep);
                nw[t] = max_u8x4(cur[t], w[t]);
                chg |= nw[t] ^ cur[t];
            }
            if (bad) atomicMin(err, (unsigned long long)idx[k]);
            int *__restrict__ drow = dl + ((j + k) << 6);  // (only touched where something changed: j + k < e there)
            if (WAVE_UNIT) {
                if (__ballot(chg != 0)) {
                    if (chg) {
#pragma unroll
                        for (int t = 0; t < 4; ++t) {
                            if (nw[t] == cur[t]) continue;
#pragma unroll
                            for (int y = 0; y < 32; y += 8) {
                                const uint32_t ob = (cur[t] >> y) & 0xFFu, nb = (nw[t] >> y) & 0xFFu;
                                if (ob != nb) {
                                    atomicAdd(&bins[wave][ob & 63], -1);
                                    atomicAdd(&bins[wave][nb & 63], 1);
                                }
                            }
                        }
                    }
                    // the wave's LDS operations complete in order; the fence keeps the compiler to that order too
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                    const int d = atomicExch(&bins[wave][lane], 0);
                    if (d) atomicAdd(&drow[lane], d);
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            } else if (chg) {
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (nw[t] == cur[t]) continue;
#pragma unroll
                    for (int y = 0; y < 32; y += 8) {
                        const uint32_t ob = (cur[t] >> y) & 0xFFu, nb = (nw[t] >> y) & 0xFFu;
                        if (ob != nb) {
                            atomicAdd(&drow[ob & 63], -1);
                            atomicAdd(&drow[nb & 63], 1);
                        }
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < 4; ++t) cur[t] = nw[t];
        }
    }
}

// Lane q owns bytes [16 q, 16 q + 16) of the flat [orders][2^p]; the rows (o * nseg + s) of `start`, s = 0 .. nseg - 1, hold the
// unions of the order's segments and leave as the unions of the segments in front of each.
__global__ __launch_bounds__(256) void k_curve_starts(uint8_t *__restrict__ start, int p, uint32_t nseg, uint64_t orders)
{
    const uint64_t q = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t o = (q << 4) >> p;
    if (o >= orders) return;
    const uint64_t off = (q << 4) & (((uint64_t)1 << p) - 1);
    uint8_t *row = start + ((o * nseg) << p) + off;
    uint32_t acc[4] = {0, 0, 0, 0};
    for (uint32_t s = 0; s < nseg; ++s, row += (uint64_t)1 << p) {
        const uint4 t = *(const uint4 *)row;
        *(uint4 *)row = make_uint4(acc[0], acc[1], acc[2], acc[3]);
        acc[0] = max_u8x4(acc[0], t.x), acc[1] = max_u8x4(acc[1], t.y), acc[2] = max_u8x4(acc[2], t.z), acc[3] = max_u8x4(acc[3], t.w);
    }
}

// one wave per chunk x = o * nchunk + c of kScanChunk steps, lane = bin: sums[x][v] = the chunk's deltas of bin v
__global__ __launch_bounds__(256) void k_curve_scan_sums(const int *__restrict__ delta, uint64_t len, uint32_t nchunk, uint64_t nx,
                                                         int *__restrict__ sums)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t x = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (x >= nx) return;
    const uint64_t o = x / nchunk, c = x - o * nchunk;
    const uint64_t i0 = c * kScanChunk, i1 = i0 + kScanChunk < len ? i0 + kScanChunk : len;
    const int *__restrict__ d = delta + ((o * len) << 6) + lane;
    int acc = 0;
    uint64_t i = i0;
    for (; i + kScanLoads <= i1; i += kScanLoads) {
        int t[kScanLoads];
#pragma unroll
        for (int k = 0; k < kScanLoads; ++k) t[k] = d[(i + k) << 6];
#pragma unroll
        for (int k = 0; k < kScanLoads; ++k) acc += t[k];
    }
    for (; i < i1; ++i) acc += d[i << 6];
    sums[(x << 6) + lane] = acc;
}

// one wave per order, lane = bin: the chunk sums of the order become the sums of the chunks in front of each, in place
__global__ __launch_bounds__(256) void k_curve_scan_offsets(int *__restrict__ sums, uint32_t nchunk, uint64_t orders)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t o = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= orders) return;
    int *s = sums + ((o * nchunk) << 6) + lane;
    int acc = 0;
    uint32_t c = 0;
    for (; c + kScanLoads <= nchunk; c += kScanLoads) {
        int t[kScanLoads];
#pragma unroll
        for (int k = 0; k < kScanLoads; ++k) t[k] = s[(uint64_t)(c + k) << 6];
#pragma unroll
        for (int k = 0; k < kScanLoads; ++k) {
            s[(uint64_t)(c + k) << 6] = acc;
            acc += t[k];
        }
    }
    for (; c < nchunk; ++c) {
        const int t = s[(uint64_t)c << 6];
        s[(uint64_t)c << 6] = acc;
        acc += t;
    }
}

// one wave per chunk, lane = bin: the running histogram of every step of the chunk, from base + the chunk's offset
// (offs == nullptr: one chunk per order), as CT counters for launch_pairs_card and, with hist != nullptr, as uint32
template <typename CT>
__global__ __launch_bounds__(256) void k_curve_scan(const int *__restrict__ delta, const int *__restrict__ offs, uint64_t len,
                                                    uint32_t nchunk, uint64_t nx, int p, CT *__restrict__ cnt, uint32_t *__restrict__ hist)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t x = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (x >= nx) return;
    const uint64_t o = x / nchunk, c = x - o * nchunk;
    const uint64_t i0 = c * kScanChunk, i1 = i0 + kScanChunk < len ? i0 + kScanChunk : len;
    const uint64_t base = ((o * len) << 6) + lane;
    uint32_t run = (lane == 0 ? 1u << p : 0u) + (offs ? (uint32_t)offs[(x << 6) + lane] : 0u);
    uint64_t i = i0;
    for (; i + kScanLoads <= i1; i += kScanLoads) {
        int t[kScanLoads];
#pragma unroll
        for (int k = 0; k < kScanLoads; ++k) t[k] = delta[base + ((i + k) << 6)];
#pragma unroll
        for (int k = 0; k < kScanLoads; ++k) {
            run += (uint32_t)t[k];
            cnt[base + ((i + k) << 6)] = (CT)run;
            if (hist) hist[base + ((i + k) << 6)] = run;
        }
    }
    for (; i < i1; ++i) {
        run += (uint32_t)delta[base + (i << 6)];
        cnt[base + (i << 6)] = (CT)run;
        if (hist) hist[base + (i << 6)] = run;
    }
}

}  // namespace

hipError_t launch_curve_walk(hipStream_t st, const uint8_t *regs, uint64_t n, int p, const uint32_t *ord, uint64_t len, uint64_t S,
                             uint64_t nseg, uint64_t orders, const uint8_t *start, int *delta, unsigned long long *err)
{
    const uint64_t nunits = orders * nseg;
    if (!nunits) return hipSuccess;
    const uint64_t lanes = (nunits << p) >> 4, blocks = (lanes + 255) / 256;
    if (nunits > 0x7FFFFFFFull || blocks > 0x7FFFFFFFull || (nseg > 1 && !start)) return hipErrorInvalidValue;
    if (p >= 10)
        hipLaunchKernelGGL(k_curve_walk<true>, dim3((uint32_t)blocks), dim3(256), 0, st, regs, n, p, ord, len, S, (uint32_t)nseg,
                           (uint32_t)nunits, start, delta, err);
    else
        hipLaunchKernelGGL(k_curve_walk<false>, dim3((uint32_t)blocks), dim3(256), 0, st, regs, n, p, ord, len, S, (uint32_t)nseg,
                           (uint32_t)nunits, start, delta, err);
    return hipGetLastError();
}

hipError_t launch_curve_starts(hipStream_t st, uint8_t *start, int p, uint64_t nseg, uint64_t orders)
{
    if (!orders || nseg < 2) return hipSuccess;
    const uint64_t lanes = (orders << p) >> 4, blocks = (lanes + 255) / 256;
    if (nseg > 0x7FFFFFFFull || blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_curve_starts, dim3((uint32_t)blocks), dim3(256), 0, st, start, p, (uint32_t)nseg, orders);
    return hipGetLastError();
}

hipError_t launch_curve_scan(hipStream_t st, const int *delta, int *sums, uint64_t len, uint64_t orders, int p, void *cnt, uint32_t *hist)
{
    if (!orders || !len) return hipSuccess;
    const uint64_t nchunk = (len + kScanChunk - 1) / kScanChunk, nx = orders * nchunk;
    if (nchunk > 0x7FFFFFFFull || (nx + 3) / 4 > 0x7FFFFFFFull || (nchunk > 1 && !sums)) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((nx + 3) / 4));
    const int *offs = nullptr;
    if (nchunk > 1) {
        hipLaunchKernelGGL(k_curve_scan_sums, grid, dim3(256), 0, st, delta, len, (uint32_t)nchunk, nx, sums);
        hipLaunchKernelGGL(k_curve_scan_offsets, dim3((uint32_t)((orders + 3) / 4)), dim3(256), 0, st, sums, (uint32_t)nchunk, orders);
        offs = sums;
    }
    if (p <= kPairsMaxP16)
        hipLaunchKernelGGL(k_curve_scan<uint16_t>, grid, dim3(256), 0, st, delta, offs, len, (uint32_t)nchunk, nx, p, (uint16_t *)cnt, hist);
    else
        hipLaunchKernelGGL(k_curve_scan<uint32_t>, grid, dim3(256), 0, st, delta, offs, len, (uint32_t)nchunk, nx, p, (uint32_t *)cnt, hist);
    return hipGetLastError();
}

}  // namespace dsh
