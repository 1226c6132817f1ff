// cluster.hip -- dsh_cluster_threshold*, dsh_cluster_pairs, dsh_cluster_csr: connected components on the device
// (DESIGN.md 4.10).  The threshold forms are the band walk of bands.h -- the band rule and the band buffer of
// dsh_dist_threshold*, the dense path unchanged -- with k_cc_band in the place of count / scan / emit: a passing value
// unites its row and its column in a union-find (kernels_cluster.hip, uf.h) and is never written anywhere.  No host wait between bands; one wait at the end reads the error word and the root
// count.  The pairs and CSR forms run the same union-find over a caller's graph and need no sketches.
#include <algorithm>

#include "bands.h"

using namespace dsh;

namespace {

struct CcState {  // cc_state on the device
    unsigned long long n_roots;
    uint32_t err, pad_;
};

}  // namespace

namespace dsh {  // (ctx.h: dsh_linkage_* partitions by the same components)

int cc_begin(dsh_ctx *c, uint64_t n)
{
    HIPCHK(c, c->cc.parent.ensure(std::max<uint64_t>(n, 1) * sizeof(uint32_t)));
    HIPCHK(c, c->cc.state.ensure(sizeof(CcState)));
    HIPCHK(c, hipMemsetAsync(c->cc.state.ptr, 0, sizeof(CcState), c->stream));
    HIPCHK(c, launch_cc_init(c->stream, (uint32_t *)c->cc.parent.ptr, n));
    return DSH_OK;
}

uint32_t *cc_err(dsh_ctx *c) { return &((CcState *)c->cc.state.ptr)->err; }
uint32_t cc_cap(uint64_t n) { return (uint32_t)std::min<uint64_t>(n + 1, 0xFFFFFFFFull); }

// labels and the root count; the one wait of a call.  d_labels: the caller's device buffer, or nullptr for h_labels (host)
int cc_finish(dsh_ctx *c, uint64_t n, uint32_t *d_labels, uint32_t *h_labels, uint64_t *n_clusters)
{
    if (!d_labels) {
        HIPCHK(c, c->cc.labels.ensure(std::max<uint64_t>(n, 1) * sizeof(uint32_t)));
        d_labels = (uint32_t *)c->cc.labels.ptr;
    }
    CcState *st = (CcState *)c->cc.state.ptr;
    HIPCHK(c, launch_cc_labels(c->stream, (uint32_t *)c->cc.parent.ptr, n, cc_cap(n), d_labels, (uint64_t *)&st->n_roots, &st->err));
    CcState h = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(&h, st, sizeof h, hipMemcpyDeviceToHost, c->stream));
    if (h_labels && n) HIPCHK(c, hipMemcpyAsync(h_labels, d_labels, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (h.err) return fail(c, DSH_EIO, "internal: union-find step bound exceeded (code %u)", h.err);
    if (n_clusters) *n_clusters = h.n_roots;
    return DSH_OK;
}

}  // namespace dsh

namespace {

// an earlier labelling (host [n], validated) to continue from
int cc_seed(dsh_ctx *c, uint64_t n, const uint32_t *labels_in)
{
    if (!labels_in || !n) return DSH_OK;
    HIPCHK(c, c->cc.seed.ensure(n * sizeof(uint32_t)));
    HIPCHK(c, hipMemcpyAsync(c->cc.seed.ptr, labels_in, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_cc_seed(c->stream, (uint32_t *)c->cc.parent.ptr, (const uint32_t *)c->cc.seed.ptr, n, cc_cap(n), cc_err(c)));
    return DSH_OK;
}

int run_cluster_threshold(dsh_ctx *c, int estim, int result_type, int k, float t, uint32_t *d_labels, uint32_t *h_labels,
                          uint64_t *n_clusters)
{
    const uint64_t n = c->n;
    if (n > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "%llu sketches: labels are 32-bit", (unsigned long long)n);
    if (n_clusters) *n_clusters = 0;
    if (!n) return DSH_OK;
    const int descending = measure_descending(result_type) ? 1 : 0;
    int rc = cc_begin(c, n);
    if (rc) return rc;
    BandQuery bq;
    bq.estim = estim, bq.result_type = result_type, bq.k = k;
    bq.re = n;
    rc = for_each_band(c, bq, [&](const ThrRows &g, const float *vals, uint64_t) -> int {
        const hipError_t e = launch_cc_band(c->stream, vals, g, t, descending, (uint32_t *)c->cc.parent.ptr, cc_cap(n), cc_err(c));
        return e == hipSuccess ? DSH_OK : fail(c, DSH_EIO, "k_cc_band: %s", hipGetErrorString(e));
    });
    if (rc) return drain(c, rc);
    if ((rc = cc_finish(c, n, d_labels, h_labels, n_clusters))) return drain(c, rc);
    return DSH_OK;
}

// what dsh_cluster_pairs and dsh_cluster_csr check alike
int check_graph(dsh_ctx *c, uint64_t n_nodes, const uint32_t *labels_in, const uint32_t *labels_out)
{
    if (!c) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    if (n_nodes > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "%llu nodes: labels are 32-bit (at most 2^32 - 1 nodes)", (unsigned long long)n_nodes);
    if (n_nodes && !labels_out) return DSH_EINVAL;
    if (labels_in)
        for (uint64_t x = 0; x < n_nodes; ++x)
            if (labels_in[x] >= n_nodes)
                return fail(c, DSH_EINVAL, "labels_in[%llu] = %u outside [0, %llu)", (unsigned long long)x, labels_in[x], (unsigned long long)n_nodes);
    return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_cluster_threshold(dsh_ctx *c, int estim, int result_type, int k, float threshold, uint32_t *labels_out, uint64_t *n_clusters)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    if (c->n && !labels_out) return DSH_EINVAL;
    return run_cluster_threshold(c, estim, result_type, k, threshold, nullptr, labels_out, n_clusters);
}

int dsh_cluster_threshold_device(dsh_ctx *c, int estim, int result_type, int k, float threshold, void *d_labels, uint64_t *n_clusters)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    if (c->n && !d_labels) return DSH_EINVAL;
    return run_cluster_threshold(c, estim, result_type, k, threshold, (uint32_t *)d_labels, nullptr, n_clusters);
}

int dsh_cluster_pairs(dsh_ctx *c, uint64_t n_nodes, const uint32_t *lhs, const uint32_t *rhs, uint64_t n_pairs, const uint32_t *labels_in,
                      uint32_t *labels_out, uint64_t *n_clusters)
{
    int rc = check_graph(c, n_nodes, labels_in, labels_out);
    if (rc) return rc;
    if (n_pairs && (!lhs || !rhs)) return DSH_EINVAL;
    for (uint64_t x = 0; x < n_pairs; ++x)
        if (lhs[x] >= n_nodes || rhs[x] >= n_nodes)
            return fail(c, DSH_EINVAL, "pair %llu names a node outside [0, %llu)", (unsigned long long)x, (unsigned long long)n_nodes);
    if (n_clusters) *n_clusters = 0;
    if (!n_nodes) return DSH_OK;
    // the list goes through bounded scratch: 8 bytes per edge of ONE chunk (the caller's arrays outlive the call, which
    // ends with a wait, so they are uploaded as they stand)
    const uint64_t chunk = std::min<uint64_t>(c->cc.chunk, std::max<uint64_t>(n_pairs, 1));
    if (n_pairs) {
        HIPCHK(c, c->cc.lhs.ensure(chunk * sizeof(uint32_t)));
        HIPCHK(c, c->cc.rhs.ensure(chunk * sizeof(uint32_t)));
    }
    if ((rc = cc_begin(c, n_nodes)) || (rc = cc_seed(c, n_nodes, labels_in))) return drain(c, rc);
    for (uint64_t x0 = 0; x0 < n_pairs; x0 += chunk) {
        const uint64_t cnt = std::min<uint64_t>(chunk, n_pairs - x0);
        if (hipMemcpyAsync(c->cc.lhs.ptr, lhs + x0, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(c->cc.rhs.ptr, rhs + x0, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            launch_cc_edges(c->stream, (uint32_t *)c->cc.parent.ptr, (const uint32_t *)c->cc.lhs.ptr, (const uint32_t *)c->cc.rhs.ptr, cnt,
                            n_nodes, cc_cap(n_nodes), cc_err(c)) != hipSuccess)
            return drain(c, fail(c, DSH_EIO, "upload of the edge list / k_cc_edges failed"));
    }
    if ((rc = cc_finish(c, n_nodes, nullptr, labels_out, n_clusters))) return drain(c, rc);
    return DSH_OK;
}

int dsh_cluster_csr(dsh_ctx *c, uint64_t n_nodes, uint64_t row_begin, uint64_t rows, const uint64_t *row_ptr, const uint32_t *col,
                    const uint32_t *labels_in, uint32_t *labels_out, uint64_t *n_clusters)
{
    int rc = check_graph(c, n_nodes, labels_in, labels_out);
    if (rc) return rc;
    if (!slots_ok(row_begin, rows, n_nodes)) return fail(c, DSH_EINVAL, "rows out of range");
    if (rows && !row_ptr) return DSH_EINVAL;
    for (uint64_t r = 0; r < rows; ++r)
        if (row_ptr[r + 1] < row_ptr[r]) return fail(c, DSH_EINVAL, "row_ptr decreases at row %llu", (unsigned long long)r);
    const uint64_t h0 = rows ? row_ptr[0] : 0, n_hits = rows ? row_ptr[rows] - h0 : 0;  // (hit h of the call is col[h], h from row_ptr[0] on)
    if (n_hits && !col) return DSH_EINVAL;
    for (uint64_t h = 0; h < n_hits; ++h)
        if (col[h0 + h] >= n_nodes)
            return fail(c, DSH_EINVAL, "col[%llu] = %u outside [0, %llu)", (unsigned long long)(h0 + h), col[h0 + h], (unsigned long long)n_nodes);
    if (n_clusters) *n_clusters = 0;
    if (!n_nodes) return DSH_OK;
    const uint64_t chunk = std::min<uint64_t>(c->cc.chunk, std::max<uint64_t>(n_hits, 1));
    if (n_hits) {
        HIPCHK(c, c->cc.rowptr.ensure((rows + 1) * sizeof(uint64_t)));
        HIPCHK(c, c->cc.lhs.ensure(chunk * sizeof(uint32_t)));
    }
    if ((rc = cc_begin(c, n_nodes)) || (rc = cc_seed(c, n_nodes, labels_in))) return drain(c, rc);
    if (n_hits) {
        // the row pointer travels whole (8 bytes per row), the columns in chunks; the row of a hit is found on the device
        if (hipMemcpyAsync(c->cc.rowptr.ptr, row_ptr, (rows + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream) != hipSuccess)
            return drain(c, fail(c, DSH_EIO, "upload of the row pointer failed"));
        for (uint64_t x0 = 0; x0 < n_hits; x0 += chunk) {
            const uint64_t cnt = std::min<uint64_t>(chunk, n_hits - x0);
            if (hipMemcpyAsync(c->cc.lhs.ptr, col + h0 + x0, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
                launch_cc_csr(c->stream, (uint32_t *)c->cc.parent.ptr, (const uint64_t *)c->cc.rowptr.ptr, rows, row_begin,
                              (const uint32_t *)c->cc.lhs.ptr, h0 + x0, cnt, n_nodes, cc_cap(n_nodes), cc_err(c)) != hipSuccess)
                return drain(c, fail(c, DSH_EIO, "upload of the columns / k_cc_csr failed"));
        }
    }
    if ((rc = cc_finish(c, n_nodes, nullptr, labels_out, n_clusters))) return drain(c, rc);
    return DSH_OK;
}

}  // extern "C"
