// hist.hip -- dsh_dist_histogram*, dsh_dist_rect_histogram: the distribution of the values of a triangle or rectangle call
// over caller-given bin edges, optionally split by a labelling into intra-group and inter-group pairs, counted on the
// device in one dense pass.  The dense path is the producer and is not changed: the band walk of bands.h
// -- the band rule and the band buffer of dsh_dist_threshold* -- with one launch of k_hist (kernels_hist.hip) per band, which
// adds into a library-owned uint64 array zeroed at the start of the call.  No host wait between bands; one at the end.
#include <algorithm>

#include "bands.h"

using namespace dsh;

namespace {

struct HistQuery {
    int estim, result_type, k;
    int rect;
    uint64_t rb, re, cb, ce;
    const float *edges;
    uint32_t n_edges;
    const uint32_t *labels;
    uint64_t *h_counts = nullptr;  // host form
    uint64_t *d_counts = nullptr;  // device form
};

// what needs no device: DSH_OK or DSH_EINVAL with a message
int hist_check(dsh_ctx *c, const HistQuery &q)
{
    if (q.n_edges == 0 || q.n_edges > DSH_HIST_MAX_EDGES)
        return fail(c, DSH_EINVAL, "%u edges: between 1 and %d", q.n_edges, DSH_HIST_MAX_EDGES);
    if (!q.edges) return fail(c, DSH_EINVAL, "no edges");
    if (!q.h_counts && !q.d_counts) return fail(c, DSH_EINVAL, "no output for the counts");
    for (uint32_t b = 0; b < q.n_edges; ++b) {
        if (q.edges[b] != q.edges[b]) return fail(c, DSH_EINVAL, "edges[%u] is NaN", b);
        if (b && !(q.edges[b - 1] < q.edges[b]))
            return fail(c, DSH_EINVAL, "edges[%u] = %.9g is not above edges[%u] = %.9g: the edges must increase strictly", b,
                        (double)q.edges[b], b - 1, (double)q.edges[b - 1]);
    }
    if (q.estim < 0 || q.estim > 2) return fail(c, DSH_EINVAL, "bad estimator %d", q.estim);
    if (q.result_type < 0 || q.result_type > 8) return fail(c, DSH_EINVAL, "unsupported result_type %d", q.result_type);
    if (q.labels && c->n > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "%llu sketches: labels are 32-bit", (unsigned long long)c->n);
    return DSH_OK;
}

int run_hist(dsh_ctx *c, const HistQuery &q)
{
    int rc = hist_check(c, q);
    if (rc) return rc;
    const int planes = q.labels ? 2 : 1;
    const uint64_t ncnt = (uint64_t)planes * (q.n_edges + 2);
    const uint64_t rows = q.re > q.rb ? q.re - q.rb : 0, cols = q.ce > q.cb ? q.ce - q.cb : 0;
    const uint64_t pairs = q.rect ? rows * cols : dsh_tri_span(c->n, q.rb, q.re);
    if (pairs && q.k < 1) return fail(c, DSH_EINVAL, "bad k %d", q.k);
    const int descending = measure_descending(q.result_type) ? 1 : 0;
    uint64_t *d_counts = q.d_counts;
    if (!d_counts) {
        HIPCHK(c, c->hs.counts.ensure(ncnt * sizeof(uint64_t)));
        d_counts = (uint64_t *)c->hs.counts.ptr;
    }
    if (c->hs.cus <= 0) {  // the residency bound of k_hist's grid (plan::hist_grid)
        int cus = 0;
        HIPCHK(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        c->hs.cus = std::max(cus, 1);
    }
    HIPCHK(c, c->hs.edges.ensure(q.n_edges * sizeof(float)));
    if (q.labels && c->n) HIPCHK(c, c->hs.labels.ensure(c->n * sizeof(uint32_t)));
    // from here on work is queued: a failure drains the stream
    if (hipMemsetAsync(d_counts, 0, ncnt * sizeof(uint64_t), c->stream) != hipSuccess) return drain(c, fail(c, DSH_EIO, "clearing the counts failed"));
    if (pairs) {
        const float *d_edges = (const float *)c->hs.edges.ptr;
        const uint32_t *d_labels = q.labels ? (const uint32_t *)c->hs.labels.ptr : nullptr;
        // (pageable sources: the runtime has taken its copy of them when the call returns)
        if (hipMemcpyAsync(c->hs.edges.ptr, q.edges, q.n_edges * sizeof(float), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            (q.labels && hipMemcpyAsync(c->hs.labels.ptr, q.labels, c->n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream) != hipSuccess))
            return drain(c, fail(c, DSH_EIO, "upload of the edges or labels failed"));
        BandQuery bq;
        bq.estim = q.estim, bq.result_type = q.result_type, bq.k = q.k, bq.rect = q.rect;
        bq.rb = q.rb, bq.re = q.re, bq.cb = q.cb, bq.ce = q.ce;
        rc = for_each_band(c, bq, [&](const ThrRows &g, const float *vals, uint64_t) -> int {
            const hipError_t e = launch_hist(c->stream, vals, g, d_edges, q.n_edges, d_labels, descending, (uint32_t)c->hs.cus, d_counts);
            return e == hipSuccess ? DSH_OK : fail(c, DSH_EIO, "k_hist: %s", hipGetErrorString(e));
        });
        if (rc) return drain(c, rc);
    }
    if (q.h_counts && hipMemcpyAsync(q.h_counts, d_counts, ncnt * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream) != hipSuccess)
        return drain(c, fail(c, DSH_EIO, "copy of the counts failed"));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
}

int tri_hist(dsh_ctx *c, int estim, int result_type, int k, uint64_t rb, uint64_t re, const float *edges, uint32_t n_edges,
             const uint32_t *labels, uint64_t *h_counts, uint64_t *d_counts)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    if (re > c->n) re = c->n;
    HistQuery q;
    q.estim = estim, q.result_type = result_type, q.k = k, q.rect = 0;
    q.rb = rb, q.re = std::max(rb, re), q.cb = q.ce = 0;
    if (q.rb > c->n) q.rb = q.re = c->n;
    q.edges = edges, q.n_edges = n_edges, q.labels = labels;
    q.h_counts = h_counts, q.d_counts = d_counts;
    return run_hist(c, q);
}

}  // namespace

extern "C" {

int dsh_dist_histogram(dsh_ctx *c, int estim, int result_type, int k, uint64_t rb, uint64_t re, const float *edges, uint32_t n_edges,
                       const uint32_t *labels, uint64_t *counts_out)
{
    return tri_hist(c, estim, result_type, k, rb, re, edges, n_edges, labels, counts_out, nullptr);
}

int dsh_dist_histogram_device(dsh_ctx *c, int estim, int result_type, int k, uint64_t rb, uint64_t re, const float *edges,
                              uint32_t n_edges, const uint32_t *labels, void *d_counts)
{
    return tri_hist(c, estim, result_type, k, rb, re, edges, n_edges, labels, nullptr, (uint64_t *)d_counts);
}

int dsh_dist_rect_histogram(dsh_ctx *c, int estim, int result_type, int k, uint64_t qb, uint64_t qe, uint64_t rb, uint64_t re,
                            const float *edges, uint32_t n_edges, const uint32_t *labels, uint64_t *counts_out)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    if (qe > c->n || re > c->n) return fail(c, DSH_EINVAL, "slots out of range");
    HistQuery q;
    q.estim = estim, q.result_type = result_type, q.k = k, q.rect = 1;
    q.rb = qb, q.re = std::max(qb, qe), q.cb = rb, q.ce = std::max(rb, re);
    q.edges = edges, q.n_edges = n_edges, q.labels = labels;
    q.h_counts = counts_out;
    return run_hist(c, q);
}

}  // extern "C"
