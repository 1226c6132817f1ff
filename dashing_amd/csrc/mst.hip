// mst.hip -- dsh_mst, dsh_mst_tri, dsh_mst_linkage: the minimum spanning tree of the pair values on the device, which is the
// single-linkage dendrogram (include/dashing_hip.h has the contract, mst.h the step logic).  Borůvka rounds
// over the band walk of bands.h: per round the labels of the union-find of cluster.hip, one k_mst_band per band, the two
// picks, the emit (kernels_mst.hip) and ONE small read of the edge count, which is the round's only wait.  Where the whole
// triangle is one band it is computed (or uploaded) once and walked again by every round; else every round recomputes (or
// uploads again) its bands.  The edges come to the host once, at the end, and are sorted there by the total order.
#include <algorithm>

#include "bands.h"
#include "mst.h"

using namespace dsh;

namespace {

struct MstState {  // mst.state on the device
    unsigned long long count;  // edges so far
    unsigned long long roots;  // what the rounds' k_cc_labels count: not read
};

// where the values come from and the band walk over either source: bands.h
using MstSource = BandSource;
template <class F>
int mst_walk(dsh_ctx *c, uint64_t n, const MstSource &s, F &&per_band)
{
    return for_each_source_band(c, n, s, per_band);
}

int mst_rounds(dsh_ctx *c, uint64_t n, const MstSource &s, int descending, float cutoff, uint64_t *count_out)
{
    const size_t w32 = n * sizeof(uint32_t), w64 = n * sizeof(uint64_t);
    HIPCHK(c, c->mst.best.ensure(w64));
    HIPCHK(c, c->mst.ckey.ensure(w32));
    HIPCHK(c, c->mst.cedge.ensure(w64));
    HIPCHK(c, c->mst.elhs.ensure(w32));
    HIPCHK(c, c->mst.erhs.ensure(w32));
    HIPCHK(c, c->mst.ekey.ensure(w32));
    HIPCHK(c, c->mst.state.ensure(sizeof(MstState)));
    HIPCHK(c, c->cc.labels.ensure(w32));
    MstState *st = (MstState *)c->mst.state.ptr;
    HIPCHK(c, hipMemsetAsync(st, 0, sizeof *st, c->stream));
    uint32_t *parent = (uint32_t *)c->cc.parent.ptr, *labels = (uint32_t *)c->cc.labels.ptr, *ckey = (uint32_t *)c->mst.ckey.ptr;
    uint64_t *best_v = (uint64_t *)c->mst.best.ptr, *cedge = (uint64_t *)c->mst.cedge.ptr;
    const MstEdges edges = {(uint32_t *)c->mst.elhs.ptr, (uint32_t *)c->mst.erhs.ptr, (uint32_t *)c->mst.ekey.ptr, &st->count, n - 1};
    // where the first round's walk saw ONE band, its values stay in thr_vals and the later rounds walk them again
    ThrRows kept;
    uint64_t bands_seen = 0;
    bool have_kept = false;
    auto per_band = [&](const ThrRows &g, const float *vals, uint64_t) -> int {
        if (!have_kept) kept = g, ++bands_seen;
        DeviceTimer tm(c, c->stream);
        const hipError_t e = launch_mst_band(c->stream, vals, g, cutoff, descending, labels, best_v);
        tm.stop(c->mst.band_ms, true);
        return e == hipSuccess ? DSH_OK : fail(c, DSH_EIO, "k_mst_band: %s", hipGetErrorString(e));
    };
    uint64_t total = 0;
    for (;;) {
        HIPCHK(c, launch_cc_labels(c->stream, parent, n, cc_cap(n), labels, (uint64_t *)&st->roots, cc_err(c)));
        HIPCHK(c, hipMemsetAsync(best_v, 0, w64, c->stream));
        HIPCHK(c, hipMemsetAsync(ckey, 0, w32, c->stream));
        HIPCHK(c, hipMemsetAsync(cedge, 0xFF, w64, c->stream));
        int rc = have_kept ? per_band(kept, (const float *)c->thr_vals.ptr, 0) : mst_walk(c, n, s, per_band);
        if (rc) return rc;
        have_kept = bands_seen == 1;
        HIPCHK(c, launch_mst_pick(c->stream, best_v, labels, ckey, cedge, n));
        HIPCHK(c, launch_mst_emit(c->stream, labels, ckey, cedge, n, parent, cc_cap(n), cc_err(c), edges));
        unsigned long long count = 0;
        HIPCHK(c, hipMemcpyAsync(&count, &st->count, sizeof count, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (count > n - 1) return fail(c, DSH_EIO, "internal: mst edge count %llu exceeds n - 1", count);
        if (count == total) break;
        total = count;
        if ((uint32_t)++c->mst.rounds_last > kMstMaxRounds) return fail(c, DSH_EIO, "internal: mst round bound exceeded");
        if (total == n - 1) break;  // a spanning tree: nothing is left to offer
    }
    *count_out = total;
    return DSH_OK;
}

int run_mst(dsh_ctx *c, uint64_t n, const MstSource &s, int descending, float cutoff, uint32_t *lhs_out, uint32_t *rhs_out, float *val_out,
            uint64_t *n_edges, uint32_t *labels_out)
{
    if (n_edges) *n_edges = 0;
    c->mst.rounds_last = 0;
    c->mst.band_ms = 0;
    if (n > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "%llu nodes: slots and labels are 32-bit (at most 2^32 - 1)", (unsigned long long)n);
    if (n >= 2 && (!lhs_out || !rhs_out || !val_out || !n_edges)) return fail(c, DSH_EINVAL, "a NULL output for %llu nodes", (unsigned long long)n);
    if (!n) return DSH_OK;
    int rc = cc_begin(c, n);
    if (rc) return drain(c, rc);
    uint64_t total = 0;
    if (n >= 2 && (rc = mst_rounds(c, n, s, descending, cutoff, &total))) return drain(c, rc);
    std::vector<uint32_t> h(3 * total);
    if (total) {
        HIPCHK(c, hipMemcpyAsync(h.data(), c->mst.elhs.ptr, total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(h.data() + total, c->mst.erhs.ptr, total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(h.data() + 2 * total, c->mst.ekey.ptr, total * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    }
    uint64_t n_clusters = 0;
    if ((rc = cc_finish(c, n, nullptr, labels_out, &n_clusters))) return drain(c, rc);  // the wait; the union-find's error word
    if (n_clusters + total != n) return fail(c, DSH_EIO, "internal: %llu mst edges but %llu components of %llu nodes", (unsigned long long)total, (unsigned long long)n_clusters, (unsigned long long)n);
    std::vector<MstEdge> e(total);
    for (uint64_t x = 0; x < total; ++x) e[x] = MstEdge{h[2 * total + x], h[x], h[total + x]};
    if (total) mst_sorted_out(e, descending, lhs_out, rhs_out, val_out);
    if (n_edges) *n_edges = total;
    return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_mst(dsh_ctx *c, int estim, int result_type, int k, float cutoff, uint32_t *lhs_out, uint32_t *rhs_out, float *val_out, uint64_t *n_edges,
            uint32_t *labels_out)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    MstSource s;
    s.estim = estim, s.result_type = result_type, s.k = k;
    return run_mst(c, c->n, s, measure_descending(result_type) ? 1 : 0, cutoff, lhs_out, rhs_out, val_out, n_edges, labels_out);
}

int dsh_mst_tri(dsh_ctx *c, uint64_t n_nodes, const float *tri, int descending, float cutoff, uint32_t *lhs_out, uint32_t *rhs_out,
                float *val_out, uint64_t *n_edges, uint32_t *labels_out)
{
    if (!c) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    reset_prof(c);
    if (n_nodes >= 2 && n_nodes <= 0xFFFFFFFFull && !tri) return fail(c, DSH_EINVAL, "no values for %llu nodes", (unsigned long long)n_nodes);
    MstSource s;
    s.tri = tri;
    return run_mst(c, n_nodes, s, descending ? 1 : 0, cutoff, lhs_out, rhs_out, val_out, n_edges, labels_out);
}

int dsh_mst_linkage(uint64_t n_nodes, const uint32_t *lhs, const uint32_t *rhs, const float *val, uint64_t n_edges, uint32_t *za, uint32_t *zb,
                    float *zv, uint32_t *zsize)
{
    if (n_edges && (!lhs || !rhs || !val || !za || !zb || !zv || !zsize)) return DSH_EINVAL;
    return mst_linkage(n_nodes, lhs, rhs, val, n_edges, za, zb, zv, zsize) ? DSH_OK : DSH_EINVAL;
}

}  // extern "C"
