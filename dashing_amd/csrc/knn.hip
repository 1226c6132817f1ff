// knn.hip -- dsh_knn: k nearest neighbours per sketch (perform_nns / nndist_loop, src/sketch_and_cmp.h:642-783),
// and its selection kernels: k_topk (one pass over a matrix), k_topk_merge / k_fill_knn_state (band-wise running lists).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "ctx.h"

namespace dsh {

// k best columns of every row of a row-major [rows][ncols] block (perform_nns,
// src/sketch_and_cmp.h:642-697, without its heaps and mutexes): one wave per row, nn selection
// passes; pass t takes the best element that comes strictly after pass t-1's pick in the total
// order (value best-first, then column index ascending), so nothing is mutated and ties are
// deterministic.  NaN ranks last.  self_col (or ~0) is skipped.
__global__ __launch_bounds__(256) void k_topk(const float *__restrict__ vals, uint64_t rows,
                                               uint64_t ncols, uint64_t row0, uint64_t col0,
                                               int descending, uint32_t nn, int exclude_self,
                                               uint32_t *__restrict__ idx_out,
                                               float *__restrict__ val_out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float *v = vals + r * ncols;
    const float worst = descending ? -__builtin_huge_valf() : __builtin_huge_valf();
    const uint64_t self = exclude_self ? row0 + r - col0 : ~0ull;  // column of the row's own sketch
    // order: a before b  <=>  a.val better than b.val, or equal and a.idx < b.idx
    auto before = [descending](float av, uint32_t ai, float bv, uint32_t bi) {
        if (av != bv) return descending ? av > bv : av < bv;
        return ai < bi;
    };
    float pv = descending ? __builtin_huge_valf() : -__builtin_huge_valf();  // "before everything"
    uint32_t pi = 0;
    bool first = true;
    for (uint32_t t = 0; t < nn; ++t) {
        float bv = worst;
        uint32_t bi = 0xFFFFFFFFu;
        for (uint64_t j = lane; j < ncols; j += 64) {
            if (j == self) continue;
            float x = v[j];
            if (x != x) x = worst;
            const uint32_t ji = (uint32_t)j;
            if (!first && !before(pv, pi, x, ji)) continue;  // not after the previous pick
            if (bi == 0xFFFFFFFFu || before(x, ji, bv, bi)) {
                bv = x;
                bi = ji;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ov = __shfl_xor(bv, d, 64);
            const uint32_t oi = __shfl_xor(bi, d, 64);
            if (oi != 0xFFFFFFFFu && (bi == 0xFFFFFFFFu || before(ov, oi, bv, bi))) {
                bv = ov;
                bi = oi;
            }
        }
        if (lane == 0) {
            idx_out[r * nn + t] = bi == 0xFFFFFFFFu ? 0xFFFFFFFFu : (uint32_t)(bi + col0);
            val_out[r * nn + t] = bi == 0xFFFFFFFFu ? worst : v[bi];
        }
        pv = bv;
        pi = bi;
        first = false;
        if (bi == 0xFFFFFFFFu) {  // fewer candidates than nn: fill the rest
            for (uint32_t u = t + 1; u < nn; ++u)
                if (lane == 0) {
                    idx_out[r * nn + u] = 0xFFFFFFFFu;
                    val_out[r * nn + u] = worst;
                }
            break;
        }
    }
}

hipError_t launch_topk(hipStream_t st, const float *vals, uint64_t rows, uint64_t ncols,
                       uint64_t row0, uint64_t col0, int descending, uint32_t nn,
                       int exclude_self, uint32_t *idx_out, float *val_out)
{
    if (rows == 0 || nn == 0) return hipSuccess;
    hipLaunchKernelGGL(k_topk, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, st, vals, rows,
                       ncols, row0, col0, descending, nn, exclude_self, idx_out, val_out);
    return hipGetLastError();
}

// Nearest neighbours without the n x n matrix (perform_nns, src/sketch_and_cmp.h:642-697, whose heaps take every pair
// as it is computed): the triangle is computed in bands of tile rows of the key-ordered layout; k_finalize leaves a
// band's values twice -- V[r][t] (row = band row r, column = plane column t > b0 + r) and Vt[t][r] (row = plane column
// t, column = band row r with b0 + r < t) -- and this kernel folds each row's new candidates into the running list of
// that row's sketch: one wave per row, nn selection passes over (running list) U (candidates) in the total order of
// k_topk (value best-first, then sketch index ascending; NaN last), every candidate carrying its ORIGINAL sketch index.
//   mode 0: rows r in [0, rows) of V (leading dimension ld): sketch perm[b0 + r], candidates t in (b0 + r, ncols)
//   mode 1: rows t in (b0, ncols) of Vt (leading dimension = band rows): sketch perm[t], candidates r in [0, min(rows, t - b0))
// state: idx[n][nn] / val[n][nn] by original sketch index, initialised to (0xFFFFFFFF, worst).
__global__ __launch_bounds__(256) void k_topk_merge(const float *__restrict__ vals, uint64_t ld, int mode, uint64_t b0,
                                                     uint64_t rows, uint64_t ncols, const uint32_t *__restrict__ perm,
                                                     int descending, uint32_t nn, uint32_t *__restrict__ st_idx,
                                                     float *__restrict__ st_val)
{
    extern __shared__ __attribute__((aligned(8))) unsigned char tk_raw[];  // per wave: nn x (idx, val) of the running list
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t *ri = reinterpret_cast<uint32_t *>(tk_raw) + (size_t)wave * 2 * nn;
    float *rv = reinterpret_cast<float *>(ri + nn);
    const uint64_t w = (uint64_t)blockIdx.x * 4 + wave;
    uint64_t srow, c_begin, c_end;  // plane column of the row's sketch; candidate columns of this row
    const float *v;
    if (mode == 0) {
        if (w >= rows) return;
        srow = b0 + w;
        c_begin = srow + 1;
        c_end = ncols;
        v = vals + w * ld;
    } else {
        srow = b0 + 1 + w;
        if (srow >= ncols) return;
        c_begin = 0;
        c_end = srow - b0 < rows ? srow - b0 : rows;
        v = vals + srow * ld;
    }
    const uint32_t self = perm ? perm[srow] : (uint32_t)srow;
    const float worst = descending ? -__builtin_huge_valf() : __builtin_huge_valf();
    for (uint32_t t = lane; t < nn; t += 64) {
        ri[t] = st_idx[(uint64_t)self * nn + t];
        rv[t] = st_val[(uint64_t)self * nn + t];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    auto before = [descending](float av, uint32_t ai, float bv, uint32_t bi) {
        if (av != bv) return descending ? av > bv : av < bv;
        return ai < bi;
    };
    float pv = descending ? __builtin_huge_valf() : -__builtin_huge_valf();
    uint32_t pi = 0;
    bool first = true;
    for (uint32_t t = 0; t < nn; ++t) {
        float bv = worst, braw = worst;  // bv: the value the order uses (NaN ranks as the worst), braw: what is reported
        uint32_t bi = 0xFFFFFFFFu;
        auto offer = [&](float raw, uint32_t id) {
            const float x = raw != raw ? worst : raw;
            if (!first && !before(pv, pi, x, id)) return;  // not after the previous pick
            if (bi == 0xFFFFFFFFu || before(x, id, bv, bi)) {
                bv = x;
                braw = raw;
                bi = id;
            }
        };
        for (uint32_t u = lane; u < nn; u += 64)
            if (ri[u] != 0xFFFFFFFFu) offer(rv[u], ri[u]);
        for (uint64_t c = c_begin + lane; c < c_end; c += 64) {
            const uint64_t sc = mode == 0 ? c : b0 + c;  // plane column of the candidate
            offer(v[c], perm ? perm[sc] : (uint32_t)sc);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ov = __shfl_xor(bv, d, 64), oraw = __shfl_xor(braw, d, 64);
            const uint32_t oi = __shfl_xor(bi, d, 64);
            if (oi != 0xFFFFFFFFu && (bi == 0xFFFFFFFFu || before(ov, oi, bv, bi))) {
                bv = ov;
                braw = oraw;
                bi = oi;
            }
        }
        if (lane == 0) {
            st_idx[(uint64_t)self * nn + t] = bi;
            st_val[(uint64_t)self * nn + t] = bi == 0xFFFFFFFFu ? worst : braw;  // (a NaN stays a NaN, as k_topk reports it)
        }
        pv = bv;
        pi = bi;
        first = false;
        if (bi == 0xFFFFFFFFu) {  // fewer candidates than nn: the rest stays empty
            for (uint32_t u = t + 1 + lane; u < nn; u += 64) {
                st_idx[(uint64_t)self * nn + u] = 0xFFFFFFFFu;
                st_val[(uint64_t)self * nn + u] = worst;
            }
            break;
        }
    }
}

__global__ __launch_bounds__(256) void k_fill_knn_state(uint32_t *__restrict__ idx, float *__restrict__ val, uint64_t cnt, float worst)
{
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < cnt) {
        idx[t] = 0xFFFFFFFFu;
        val[t] = worst;
    }
}

hipError_t launch_knn_state_init(hipStream_t st, uint32_t *idx, float *val, uint64_t cnt, int descending)
{
    if (cnt == 0) return hipSuccess;
    const float worst = descending ? -__builtin_huge_valf() : __builtin_huge_valf();
    hipLaunchKernelGGL(k_fill_knn_state, dim3((uint32_t)((cnt + 255) / 256)), dim3(256), 0, st, idx, val, cnt, worst);
    return hipGetLastError();
}

hipError_t launch_topk_merge(hipStream_t st, const float *vals, uint64_t ld, int mode, uint64_t b0, uint64_t rows,
                             uint64_t ncols, const uint32_t *perm, int descending, uint32_t nn, uint32_t *st_idx,
                             float *st_val)
{
    const uint64_t nrows = mode == 0 ? rows : (ncols > b0 + 1 ? ncols - b0 - 1 : 0);
    if (nrows == 0 || nn == 0) return hipSuccess;
    const size_t lds = (size_t)4 * 2 * nn * sizeof(uint32_t);
    hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void *>(k_topk_merge), lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_topk_merge, dim3((uint32_t)((nrows + 3) / 4)), dim3(256), lds, st, vals, ld, mode, b0, rows, ncols,
                       perm, descending, nn, st_idx, st_val);
    return hipGetLastError();
}

hipError_t preload_knn_kernels()
{
    hipFuncAttributes fa;
    return hipFuncGetAttributes(&fa, reinterpret_cast<const void *>(k_fill_knn_state));
}

}  // namespace dsh

using namespace dsh;

namespace {

// the selected neighbours of `rows` queries to the host; returns when they have arrived
int copy_out(dsh_ctx *c, const DevBuf &didx, const DevBuf &dval, uint64_t rows, uint32_t nn, uint32_t *idx_out, float *val_out)
{
    if (hipMemcpyAsync(idx_out, didx.ptr, rows * nn * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipMemcpyAsync(val_out, dval.ptr, rows * nn * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, DSH_EIO, "copy of neighbours failed");
    return DSH_OK;
}

// all-vs-all: every pair is computed ONCE (triangle tiles, sorted columns) and written at
// both (i,j) and (j,i) of an n x n matrix in HBM; then one selection pass per row
int knn_square(dsh_ctx *c, int estim, int result_type, int k, int descending, uint32_t nn, uint32_t *idx_out, float *val_out)
{
    const uint64_t n = c->n;
    DevBuf sq, didx, dval;  // (the call's own: freed when it leaves)
    if (sq.ensure(n * n * sizeof(float)) != hipSuccess || didx.ensure(n * nn * sizeof(uint32_t)) != hipSuccess ||
        dval.ensure(n * nn * sizeof(float)) != hipSuccess)
        return fail(c, DSH_ENOMEM, "device allocation failed");
    PairJob j = PairJob::triangle(estim, result_type, k, 0, n, 0, sq.ptr);
    j.square = 1;
    j.ksinv_double = 1;
    j.col_begin = 0, j.col_end = n;
    int rc = run_pairs(c, j);
    if (rc) return rc;
    hipError_t e = launch_topk(c->stream, (const float *)sq.ptr, n, n, 0, 0, descending, nn, 1,
                               (uint32_t *)didx.ptr, (float *)dval.ptr);
    if (e != hipSuccess) return fail(c, DSH_EIO, "k_topk: %s", hipGetErrorString(e));
    return copy_out(c, didx, dval, n, nn, idx_out, val_out);
}

// all-vs-all beyond the n x n budget: the triangle ONCE, in bands of tile rows of the key-ordered layout.  A band
// leaves its values twice (V: band rows x columns, Vt: columns x band rows -- each pair is a candidate of both its
// sketches) and two selection passes fold them into the running lists of the n sketches; nothing of size n x n
// exists (nndist_loop, src/sketch_and_cmp.h:712-783, keeps n heaps the same way).
int knn_bands(dsh_ctx *c, int estim, int result_type, int k, int descending, uint32_t nn, uint32_t *idx_out, float *val_out)
{
    const uint64_t n = c->n;
    int rc = prepare(c, estim, 1);
    if (rc) return rc;
    const uint64_t npad = c->lay.Npad;
    const uint64_t budget = std::max<uint64_t>(std::min<uint64_t>(c->knn_square_budget, (uint64_t)16 << 30), 2 * kTile * npad * sizeof(float));
    const uint64_t band = std::min<uint64_t>(npad, budget / (2 * npad * sizeof(float)) / kTile * kTile);
    // (what is still queued reads the buffers: the stream drains before they are freed, whichever way the call leaves)
    struct Drain {
        hipStream_t st;
        ~Drain() { (void)hipStreamSynchronize(st); }
    };
    DevBuf V, Vt, didx, dval;  // (the call's own: freed when it leaves)
    const Drain drain{c->stream};  // (declared last: it runs first)
    if (V.ensure(band * npad * sizeof(float)) != hipSuccess || Vt.ensure(npad * band * sizeof(float)) != hipSuccess ||
        didx.ensure(n * nn * sizeof(uint32_t)) != hipSuccess || dval.ensure(n * nn * sizeof(float)) != hipSuccess)
        return fail(c, DSH_ENOMEM, "device allocation failed");
    hipError_t e = launch_knn_state_init(c->stream, (uint32_t *)didx.ptr, (float *)dval.ptr, n * nn, descending);
    if (e != hipSuccess) return fail(c, DSH_EIO, "k_fill_knn_state: %s", hipGetErrorString(e));
    for (uint64_t b0 = 0; b0 < n; b0 += band) {
        const uint64_t b1 = std::min<uint64_t>(n, b0 + band);
        PairJob j = PairJob::triangle(estim, result_type, k, b0, b1, 0, V.ptr);
        j.sorted_rows = 1;
        j.knn = 1;
        j.ksinv_double = 1;
        j.d_out2 = (float *)Vt.ptr;
        j.knn_ld = npad;
        j.knn_rows = band;
        if ((rc = run_pairs(c, j))) return rc;
        const uint32_t *perm = (const uint32_t *)c->perm.ptr;
        e = launch_topk_merge(c->stream, (const float *)V.ptr, npad, 0, b0, b1 - b0, n, perm, descending, nn,
                              (uint32_t *)didx.ptr, (float *)dval.ptr);
        if (e == hipSuccess)
            e = launch_topk_merge(c->stream, (const float *)Vt.ptr, band, 1, b0, b1 - b0, n, perm, descending, nn,
                                  (uint32_t *)didx.ptr, (float *)dval.ptr);
        if (e != hipSuccess) return fail(c, DSH_EIO, "k_topk_merge: %s", hipGetErrorString(e));
    }
    return copy_out(c, didx, dval, n, nn, idx_out, val_out);
}

// a query range against a reference range: rectangles of at most 256 Mi values, one selection pass each
int knn_rect(dsh_ctx *c, int estim, int result_type, int k, int descending, uint64_t qb, uint64_t qe, uint64_t rb, uint64_t re,
             uint32_t nn, uint32_t *idx_out, float *val_out)
{
    const uint64_t nq = qe - qb, nr = re > rb ? re - rb : 0;
    const bool overlap = qb < re && rb < qe;
    DevBuf &rect = c->outbuf;
    const uint64_t qblock = std::max<uint64_t>(1, std::min<uint64_t>(nq, ((uint64_t)256 << 20) / std::max<uint64_t>(nr, 1)));
    HIPCHK(c, rect.ensure(std::max<uint64_t>(qblock * nr, 1) * sizeof(float)));
    DevBuf didx, dval;  // (the call's own: freed when it leaves)
    if (didx.ensure(nq * nn * sizeof(uint32_t)) != hipSuccess || dval.ensure(nq * nn * sizeof(float)) != hipSuccess)
        return fail(c, DSH_ENOMEM, "device allocation failed");
    for (uint64_t q0 = qb; q0 < qe; q0 += qblock) {
        const uint64_t q1 = std::min(qe, q0 + qblock);
        if (nr) {
            PairJob j = PairJob::rectangle(estim, result_type, k, q0, q1, rb, re, rect.ptr);
            j.ksinv_double = 1;
            int rc = run_pairs(c, j);
            if (rc) return rc;
        }
        hipError_t e = launch_topk(c->stream, (const float *)rect.ptr, q1 - q0, nr, q0, rb, descending, nn,
                                   overlap ? 1 : 0, (uint32_t *)didx.ptr + (q0 - qb) * nn,
                                   (float *)dval.ptr + (q0 - qb) * nn);
        if (e != hipSuccess) return fail(c, DSH_EIO, "k_topk: %s", hipGetErrorString(e));
    }
    return copy_out(c, didx, dval, nq, nn, idx_out, val_out);
}

}  // namespace

extern "C" {

int dsh_knn(dsh_ctx *c, int estim, int result_type, int k, uint64_t qb, uint64_t qe, uint64_t rb,
            uint64_t re, uint32_t nn, uint32_t *idx_out, float *val_out)
{
    int rc = enter(c);
    if (rc) return rc;
    if (qe > c->n || re > c->n) return fail(c, DSH_EINVAL, "slots out of range");
    reset_prof(c);
    if (qb >= qe || nn == 0) return DSH_OK;
    if (!idx_out || !val_out) return DSH_EINVAL;
    // similarity measures rank descending, distances ascending (emt2nntype, src/dashing.h:268-280)
    const int descending = measure_descending(result_type);
    const bool all_vs_all = qb == 0 && rb == 0 && qe == c->n && re == c->n && c->n > 1;
    if (all_vs_all && c->n * c->n * sizeof(float) <= c->knn_square_budget)
        return knn_square(c, estim, result_type, k, descending, nn, idx_out, val_out);
    if (all_vs_all && nn <= 1024) return knn_bands(c, estim, result_type, k, descending, nn, idx_out, val_out);
    return knn_rect(c, estim, result_type, k, descending, qb, qe, rb, re, nn, idx_out, val_out);
}

}  // extern "C"
