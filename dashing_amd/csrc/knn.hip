// knn.hip -- dsh_knn: k nearest neighbours per sketch (perform_nns / nndist_loop, src/sketch_and_cmp.h:642-783).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "ctx.h"

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
