// dbscan.hip -- dsh_dbscan_threshold*, dsh_dbscan_tri, dsh_degree_threshold*: density clusters at a threshold and the degrees
// of the threshold graph, on the device (include/dashing_hip.h has the contract, kernels_dbscan.hip the
// kernels).  Two walks over the band walk of bands.h -- the band rule and the band buffer of dsh_dist_threshold*, the dense path
// unchanged: walk 1 counts the degrees, walk 2 unites the cores in the union-find of cluster.hip and offers every non-core its
// core neighbours, then one launch writes labels, kinds and counts.  Where walk 1 saw exactly ONE band its values stay in
// thr_vals and walk 2 walks them again; else walk 2 recomputes (or uploads again) its bands: about two dense passes.  No hit is
// written anywhere, no host wait between bands; one wait at the end reads the counts and the error word.
#include <algorithm>

#include "bands.h"

using namespace dsh;

namespace {

struct DbState {  // db.state on the device
    unsigned long long n_clusters, n_noise;
    uint32_t err, pad_;
};

struct DbOut {  // each a device buffer, or a host array, or neither
    uint32_t *d_labels = nullptr, *h_labels = nullptr;
    uint8_t *d_kind = nullptr, *h_kind = nullptr;
    uint32_t *d_degree = nullptr, *h_degree = nullptr;
};

// the band walk over either source; a single node has no pair (and a NULL triangle)
template <class F>
int db_walk(dsh_ctx *c, uint64_t n, const BandSource &s, F &&per_band)
{
    return n < 2 ? DSH_OK : for_each_source_band(c, n, s, per_band);
}

// walk 1: degree[n] of the graph at t into c->db.degree.  *kept, *one_band: the geometry of the walk's band where it was the only one
int db_degrees(dsh_ctx *c, uint64_t n, const BandSource &s, int descending, float t, ThrRows *kept, bool *one_band)
{
    HIPCHK(c, c->db.degree.ensure(n * sizeof(uint32_t)));
    HIPCHK(c, hipMemsetAsync(c->db.degree.ptr, 0, n * sizeof(uint32_t), c->stream));
    uint64_t bands = 0;
    const int rc = db_walk(c, n, s, [&](const ThrRows &g, const float *vals, uint64_t) -> int {
        if (kept) *kept = g;
        ++bands;
        const hipError_t e = launch_db_degree(c->stream, vals, g, t, descending, (uint32_t *)c->db.degree.ptr);
        return e == hipSuccess ? DSH_OK : fail(c, DSH_EIO, "k_db_deg_rows / k_db_deg_cols: %s", hipGetErrorString(e));
    });
    if (one_band) *one_band = bands == 1;
    return rc;
}

int run_degree(dsh_ctx *c, int estim, int result_type, int k, float t, uint32_t *d_degree, uint32_t *h_degree)
{
    const uint64_t n = c->n;
    if (n > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "%llu sketches: degrees are 32-bit", (unsigned long long)n);
    if (n && !d_degree && !h_degree) return DSH_EINVAL;
    if (!n) return DSH_OK;
    BandSource s;
    s.estim = estim, s.result_type = result_type, s.k = k;
    int rc = db_degrees(c, n, s, measure_descending(result_type) ? 1 : 0, t, nullptr, nullptr);
    if (rc) return drain(c, rc);
    const hipError_t e = hipMemcpyAsync(d_degree ? d_degree : h_degree, c->db.degree.ptr, n * sizeof(uint32_t),
                                        d_degree ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream);
    if (e != hipSuccess) return drain(c, fail(c, DSH_EIO, "copy of the degrees: %s", hipGetErrorString(e)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
}

// the enqueues of a call behind its argument checks
int db_enqueue(dsh_ctx *c, uint64_t n, const BandSource &s, int descending, float t, uint32_t min_pts, int assign_mode, const DbOut &o,
               DbState *h)
{
    HIPCHK(c, c->db.best.ensure(n * sizeof(uint64_t)));
    HIPCHK(c, c->db.state.ensure(sizeof(DbState)));
    uint32_t *d_labels = o.d_labels;
    if (!d_labels) {
        HIPCHK(c, c->cc.labels.ensure(n * sizeof(uint32_t)));
        d_labels = (uint32_t *)c->cc.labels.ptr;
    }
    uint8_t *d_kind = o.d_kind;
    if (o.h_kind) {
        HIPCHK(c, c->db.kind.ensure(n));
        d_kind = (uint8_t *)c->db.kind.ptr;
    }
    DbState *st = (DbState *)c->db.state.ptr;
    HIPCHK(c, hipMemsetAsync(st, 0, sizeof *st, c->stream));
    HIPCHK(c, hipMemsetAsync(c->db.best.ptr, 0, n * sizeof(uint64_t), c->stream));
    int rc = cc_begin(c, n);
    if (rc) return rc;
    ThrRows kept;
    bool one_band = false;
    if ((rc = db_degrees(c, n, s, descending, t, &kept, &one_band))) return rc;
    const uint32_t *degree = (const uint32_t *)c->db.degree.ptr;
    uint32_t *parent = (uint32_t *)c->cc.parent.ptr;
    auto per_band = [&](const ThrRows &g, const float *vals, uint64_t) -> int {
        const hipError_t e = launch_db_band(c->stream, vals, g, t, descending, degree, min_pts, assign_mode == DSH_GREEDY_BEST, parent, cc_cap(n),
                                            &st->err, (uint64_t *)c->db.best.ptr);
        return e == hipSuccess ? DSH_OK : fail(c, DSH_EIO, "k_db_band: %s", hipGetErrorString(e));
    };
    // walk 2: the one band of walk 1 is still in thr_vals; else its bands are computed (or uploaded) again
    if ((rc = one_band ? per_band(kept, (const float *)c->thr_vals.ptr, 0) : db_walk(c, n, s, per_band))) return rc;
    HIPCHK(c, launch_db_labels(c->stream, parent, n, cc_cap(n), degree, (const uint64_t *)c->db.best.ptr, min_pts, d_labels, d_kind, o.d_degree,
                               (uint64_t *)&st->n_clusters, (uint64_t *)&st->n_noise, &st->err));
    HIPCHK(c, hipMemcpyAsync(h, st, sizeof *h, hipMemcpyDeviceToHost, c->stream));
    if (o.h_labels) HIPCHK(c, hipMemcpyAsync(o.h_labels, d_labels, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (o.h_kind) HIPCHK(c, hipMemcpyAsync(o.h_kind, d_kind, n, hipMemcpyDeviceToHost, c->stream));
    if (o.h_degree) HIPCHK(c, hipMemcpyAsync(o.h_degree, degree, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
}

int run_dbscan(dsh_ctx *c, uint64_t n, const BandSource &s, int descending, float t, uint32_t min_pts, int assign_mode, const DbOut &o,
               uint64_t *n_clusters, uint64_t *n_noise)
{
    if (n_clusters) *n_clusters = 0;
    if (n_noise) *n_noise = 0;
    if (n > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "%llu nodes: labels are 32-bit (at most 2^32 - 1)", (unsigned long long)n);
    if (!min_pts) return fail(c, DSH_EINVAL, "min_pts is at least 1 (a point counts itself)");
    if (assign_mode != DSH_GREEDY_FIRST && assign_mode != DSH_GREEDY_BEST) return fail(c, DSH_EINVAL, "unknown assign_mode %d", assign_mode);
    if (n && !o.d_labels && !o.h_labels) return fail(c, DSH_EINVAL, "a NULL labels output for %llu nodes", (unsigned long long)n);
    if (!n) return DSH_OK;
    DbState h = {0, 0, 0, 0};
    const int rc = db_enqueue(c, n, s, descending, t, min_pts, assign_mode, o, &h);
    if (rc) return drain(c, rc);
    if (h.err) return fail(c, DSH_EIO, "internal: union-find step bound exceeded (code %u)", h.err);
    if (n_clusters) *n_clusters = h.n_clusters;
    if (n_noise) *n_noise = h.n_noise;
    return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_dbscan_threshold(dsh_ctx *c, int estim, int result_type, int k, float threshold, uint32_t min_pts, int assign_mode,
                         uint32_t *labels_out, uint8_t *kind_out, uint32_t *degree_out, uint64_t *n_clusters, uint64_t *n_noise)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    BandSource s;
    s.estim = estim, s.result_type = result_type, s.k = k;
    DbOut o;
    o.h_labels = labels_out, o.h_kind = kind_out, o.h_degree = degree_out;
    return run_dbscan(c, c->n, s, measure_descending(result_type) ? 1 : 0, threshold, min_pts, assign_mode, o, n_clusters, n_noise);
}

int dsh_dbscan_threshold_device(dsh_ctx *c, int estim, int result_type, int k, float threshold, uint32_t min_pts, int assign_mode,
                                void *d_labels, void *d_kind, void *d_degree, uint64_t *n_clusters, uint64_t *n_noise)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    BandSource s;
    s.estim = estim, s.result_type = result_type, s.k = k;
    DbOut o;
    o.d_labels = (uint32_t *)d_labels, o.d_kind = (uint8_t *)d_kind, o.d_degree = (uint32_t *)d_degree;
    return run_dbscan(c, c->n, s, measure_descending(result_type) ? 1 : 0, threshold, min_pts, assign_mode, o, n_clusters, n_noise);
}

int dsh_dbscan_tri(dsh_ctx *c, uint64_t n_nodes, const float *tri, int descending, float threshold, uint32_t min_pts, int assign_mode,
                   uint32_t *labels_out, uint8_t *kind_out, uint32_t *degree_out, uint64_t *n_clusters, uint64_t *n_noise)
{
    if (!c) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    reset_prof(c);
    if (n_nodes >= 2 && n_nodes <= 0xFFFFFFFFull && !tri) return fail(c, DSH_EINVAL, "no values for %llu nodes", (unsigned long long)n_nodes);
    BandSource s;
    s.tri = tri;
    DbOut o;
    o.h_labels = labels_out, o.h_kind = kind_out, o.h_degree = degree_out;
    return run_dbscan(c, n_nodes, s, descending ? 1 : 0, threshold, min_pts, assign_mode, o, n_clusters, n_noise);
}

int dsh_degree_threshold(dsh_ctx *c, int estim, int result_type, int k, float threshold, uint32_t *degree_out)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    return run_degree(c, estim, result_type, k, threshold, nullptr, degree_out);
}

int dsh_degree_threshold_device(dsh_ctx *c, int estim, int result_type, int k, float threshold, void *d_degree)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    return run_degree(c, estim, result_type, k, threshold, (uint32_t *)d_degree, nullptr);
}

}  // extern "C"
