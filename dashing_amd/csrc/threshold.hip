// threshold.hip -- dsh_dist_threshold*, dsh_dist_rect_threshold: the pairs whose value passes a threshold, as CSR, without
// the dense result ever reaching the host.  The dense path is the producer and is not changed: the band walk
// of bands.h computes a band of whole rows into a library-owned device buffer, which is then counted, scanned and emitted on
// the ctx stream (kernels_threshold.hip).
#include <algorithm>
#include <cstring>

#include "bands.h"

using namespace dsh;

namespace {

struct ThrQuery {
    int estim, result_type, k;
    int rect;
    uint64_t rb, re;  // rows: triangle rows or query slots
    uint64_t cb, ce;  // rectangle: reference slots
    float t;
    // device form: the caller's buffers
    uint64_t *d_row_ptr = nullptr;
    uint32_t *d_col = nullptr;
    float *d_val = nullptr;
    uint64_t cap = 0;
    // host form
    bool host = false;
    uint64_t *h_row_ptr = nullptr;
    uint32_t **h_col = nullptr;
    float **h_val = nullptr;
};

// page-locked col/val of the host form, grown by doubling (the number of hits is only known at the end)
struct HostHits {
    uint32_t *col = nullptr;
    float *val = nullptr;
    uint64_t cap = 0;
    bool grow(uint64_t want, uint64_t used)
    {
        if (want <= cap) return true;
        const uint64_t ncap = std::max<uint64_t>(std::max<uint64_t>(want, 2 * cap), 1024);
        uint32_t *nc = (uint32_t *)dsh_alloc_host(ncap * sizeof(uint32_t));
        float *nv = (float *)dsh_alloc_host(ncap * sizeof(float));
        if (!nc || !nv) {
            dsh_free_host(nc);
            dsh_free_host(nv);
            return false;
        }
        if (used) {
            std::memcpy(nc, col, used * sizeof(uint32_t));
            std::memcpy(nv, val, used * sizeof(float));
        }
        release();
        col = nc, val = nv, cap = ncap;
        return true;
    }
    void release()
    {
        dsh_free_host(col);
        dsh_free_host(val);
        col = nullptr, val = nullptr, cap = 0;
    }
};

int run_threshold(dsh_ctx *c, const ThrQuery &q, uint64_t *n_hits)
{
    const int descending = measure_descending(q.result_type) ? 1 : 0;
    const uint64_t rows = q.re > q.rb ? q.re - q.rb : 0;
    const bool emit = q.host ? (q.h_col && q.h_val) : (q.d_col && q.d_val);
    HIPCHK(c, c->thr.total.ensure(sizeof(uint64_t)));
    uint64_t *d_total = (uint64_t *)c->thr.total.ptr;
    uint64_t *d_row_ptr = q.d_row_ptr;
    if (q.host) {
        HIPCHK(c, c->thr.rowptr.ensure((rows + 1) * sizeof(uint64_t)));
        d_row_ptr = (uint64_t *)c->thr.rowptr.ptr;
    }
    HIPCHK(c, hipMemsetAsync(d_total, 0, sizeof(uint64_t), c->stream));
    // from here on work is queued: every failure goes through the one exit below, which drains the stream and frees hh
    HostHits hh;
    uint64_t done = 0;  // (host form) hits of the bands so far
    BandQuery bq;
    bq.estim = q.estim, bq.result_type = q.result_type, bq.k = q.k, bq.rect = q.rect;
    bq.rb = q.rb, bq.re = q.re, bq.cb = q.cb, bq.ce = q.ce;
    bq.empty_bands = true;  // a row without values still has its entry of row_ptr
    int rc = for_each_band(c, bq, [&](const ThrRows &g, const float *vals, uint64_t) -> int {
        const uint64_t m = g.rows * g.nchunks;
        HIPCHK(c, c->thr.cnt.ensure(m * sizeof(uint32_t)));
        HIPCHK(c, c->thr.off.ensure((m + 1) * sizeof(uint64_t)));
        hipError_t e = launch_thr_count(c->stream, vals, g, q.t, descending, (uint32_t *)c->thr.cnt.ptr);
        if (e == hipSuccess)
            e = launch_thr_scan(c->stream, (const uint32_t *)c->thr.cnt.ptr, m, g.nchunks, (uint64_t *)c->thr.off.ptr,
                                d_row_ptr + (g.row0 - q.rb), d_total);
        if (e != hipSuccess) return fail(c, DSH_EIO, "k_thr_count/k_thr_scan: %s", hipGetErrorString(e));
        if (!emit) return DSH_OK;
        if (!q.host) {
            e = launch_thr_emit(c->stream, vals, g, q.t, descending, (const uint64_t *)c->thr.off.ptr, 0, q.cap, q.d_col, q.d_val);
            return e == hipSuccess ? DSH_OK : fail(c, DSH_EIO, "k_thr_emit: %s", hipGetErrorString(e));
        }
        // the band's total decides how much room its hits need: the one host wait per band
        uint64_t tot = 0;
        if (hipMemcpyAsync(&tot, d_total, sizeof tot, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess)
            return fail(c, DSH_EIO, "copy of the band total failed");
        const uint64_t bh = tot - done;
        if (bh) {
            HIPCHK(c, c->thr.col.ensure(bh * sizeof(uint32_t)));
            HIPCHK(c, c->thr.val.ensure(bh * sizeof(float)));
            if (!hh.grow(tot, done))  // (the stream is idle: earlier bands' copies have arrived)
                return fail(c, DSH_ENOMEM, "host allocation of %llu hits failed", (unsigned long long)tot);
            e = launch_thr_emit(c->stream, vals, g, q.t, descending, (const uint64_t *)c->thr.off.ptr, done, bh,
                                (uint32_t *)c->thr.col.ptr, (float *)c->thr.val.ptr);
            if (e != hipSuccess) return fail(c, DSH_EIO, "k_thr_emit: %s", hipGetErrorString(e));
            if (hipMemcpyAsync(hh.col + done, c->thr.col.ptr, bh * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                hipMemcpyAsync(hh.val + done, c->thr.val.ptr, bh * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
                return fail(c, DSH_EIO, "copy of the hits failed");
        }
        done = tot;
        return DSH_OK;
    });
    uint64_t total = 0;
    if (rc == DSH_OK) {
        // row_ptr[rows] = the total (also the whole of an empty range's row pointer)
        if (hipMemcpyAsync(d_row_ptr + rows, d_total, sizeof(uint64_t), hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(&total, d_total, sizeof total, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            (q.host && hipMemcpyAsync(q.h_row_ptr, d_row_ptr, (rows + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess))
            rc = fail(c, DSH_EIO, "copy of the row pointer failed");
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess && rc == DSH_OK) rc = fail(c, DSH_EIO, "hipStreamSynchronize failed");
    if (rc == DSH_OK && q.host && emit && !hh.col && !hh.grow(1, 0)) rc = fail(c, DSH_ENOMEM, "host allocation failed");  // no hits: still a pointer to free
    if (rc) {  // (the wait above has drained the stream)
        (void)hipGetLastError();
        hh.release();
        return rc;
    }
    if (n_hits) *n_hits = total;
    if (q.host && emit) {
        *q.h_col = hh.col;
        *q.h_val = hh.val;
    }
    if (!q.host && emit && total > q.cap)
        return fail(c, DSH_ERANGE, "%llu hits do not fit the capacity of %llu: row_ptr and n_hits are complete, the first %llu hits written",
                    (unsigned long long)total, (unsigned long long)q.cap, (unsigned long long)q.cap);
    return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_dist_threshold(dsh_ctx *c, int estim, int result_type, int k, uint64_t rb, uint64_t re, float threshold,
                       uint64_t *row_ptr_out, uint32_t **col_out, float **val_out, uint64_t *n_hits)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    if (!row_ptr_out) return DSH_EINVAL;
    if ((col_out == nullptr) != (val_out == nullptr)) return fail(c, DSH_EINVAL, "col_out and val_out go together");
    if (re > c->n) re = c->n;
    if (col_out) *col_out = nullptr, *val_out = nullptr;
    ThrQuery q;
    q.estim = estim, q.result_type = result_type, q.k = k, q.rect = 0;
    q.rb = rb, q.re = std::max(rb, re), q.cb = q.ce = 0;
    if (q.rb > c->n) q.rb = q.re = c->n;
    q.t = threshold;
    q.host = true;
    q.h_row_ptr = row_ptr_out, q.h_col = col_out, q.h_val = val_out;
    return run_threshold(c, q, n_hits);
}

int dsh_dist_threshold_device(dsh_ctx *c, int estim, int result_type, int k, uint64_t rb, uint64_t re, float threshold,
                              void *d_row_ptr, void *d_col, void *d_val, uint64_t cap, uint64_t *n_hits)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    if (!d_row_ptr) return DSH_EINVAL;
    if ((d_col == nullptr) != (d_val == nullptr)) return fail(c, DSH_EINVAL, "d_col and d_val go together");
    if (re > c->n) re = c->n;
    ThrQuery q;
    q.estim = estim, q.result_type = result_type, q.k = k, q.rect = 0;
    q.rb = rb, q.re = std::max(rb, re), q.cb = q.ce = 0;
    if (q.rb > c->n) q.rb = q.re = c->n;
    q.t = threshold;
    q.d_row_ptr = (uint64_t *)d_row_ptr, q.d_col = (uint32_t *)d_col, q.d_val = (float *)d_val, q.cap = cap;
    return run_threshold(c, q, n_hits);
}

int dsh_dist_rect_threshold(dsh_ctx *c, int estim, int result_type, int k, uint64_t qb, uint64_t qe, uint64_t rb, uint64_t re,
                            float threshold, uint64_t *row_ptr_out, uint32_t **col_out, float **val_out, uint64_t *n_hits)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    if (qe > c->n || re > c->n) return fail(c, DSH_EINVAL, "slots out of range");
    if (!row_ptr_out) return DSH_EINVAL;
    if ((col_out == nullptr) != (val_out == nullptr)) return fail(c, DSH_EINVAL, "col_out and val_out go together");
    if (col_out) *col_out = nullptr, *val_out = nullptr;
    ThrQuery q;
    q.estim = estim, q.result_type = result_type, q.k = k, q.rect = 1;
    q.rb = qb, q.re = std::max(qb, qe), q.cb = rb, q.ce = std::max(rb, re);
    q.t = threshold;
    q.host = true;
    q.h_row_ptr = row_ptr_out, q.h_col = col_out, q.h_val = val_out;
    return run_threshold(c, q, n_hits);
}

}  // extern "C"
