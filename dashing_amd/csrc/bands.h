// bands.h -- the band walk that dsh_dist_threshold*, dsh_cluster_threshold*, dsh_greedy_threshold*, dsh_greedy_extend* and
// the dense route of dsh_group_stats* share: rows of the packed triangle, or of a rectangle, are cut into
// bands of whole rows by the planner's rule (plan.h: tri_band_end, rect_band_rows); a band is computed by run_pairs into
// the library-owned c->thr_vals exactly as dsh_dist_rows_device / dsh_dist_rect compute it -- the dense path is the
// producer and is not changed -- and handed to the caller's kernels as a ThrRows (kernels.h, thr_walk.h).  Everything is
// enqueued on the ctx stream; no host wait of its own.  dsh_mst* and dsh_dbscan_* walk the whole triangle through
// for_each_source_band, which also takes a caller's own triangle on the host in the place of the sketches.
#pragma once
#include <algorithm>

#include "ctx.h"

namespace dsh {

// the geometry of the band [b0, b1): rows of the triangle of n sketches, or (rect) of ncols columns from col0 on
inline int thr_geometry(dsh_ctx *c, int rect, uint64_t n, uint64_t b0, uint64_t b1, uint64_t ncols, uint64_t col0, ThrRows &g)
{
    const uint64_t longest = rect ? ncols : n - 1 - b0;
    const uint64_t nchunks = std::max<uint64_t>((longest + kThrChunk - 1) / kThrChunk, 1);
    if ((nchunks + 3) / 4 > 65535) return fail(c, DSH_EINVAL, "rows of %llu values are not supported", (unsigned long long)longest);
    g.rect = rect;
    g.n = n;
    g.row0 = b0;
    g.ncols = rect ? ncols : 0;
    g.col0 = rect ? col0 : 0;
    g.rows = b1 - b0;
    g.nchunks = (uint32_t)nchunks;
    return DSH_OK;
}

// the span values of band g into c->thr_vals
inline int compute_band(dsh_ctx *c, int estim, int result_type, int k, const ThrRows &g, uint64_t span)
{
    HIPCHK(c, c->thr_vals.ensure(std::max<uint64_t>(span, 1) * sizeof(float)));
    if (!span) return DSH_OK;
    const uint64_t b1 = g.row0 + g.rows;
    return run_pairs(c, g.rect ? PairJob::rectangle(estim, result_type, k, g.row0, b1, g.col0, g.col0 + g.ncols, c->thr_vals.ptr)
                               : PairJob::triangle(estim, result_type, k, g.row0, b1, dsh_tri_span(g.n, 0, g.row0), c->thr_vals.ptr));
}

struct BandQuery {
    int estim, result_type, k;
    int rect = 0;
    uint64_t rb = 0, re = 0;        // rows: of the triangle of c->n sketches (re <= c->n), or of the rectangle
    uint64_t cb = 0, ce = 0;        // rectangle: columns
    uint64_t row_cap = kBandMaxRows;  // one more cap on the rows of a triangle band
    bool empty_bands = false;       // per_band also sees the bands without a value (an empty last row, a rectangle without columns)
};

// per_band(const ThrRows &g, const float *vals, uint64_t span) -> DSH_*: once per band, in row order, after the band's values
// were enqueued.  The first code that is not DSH_OK ends the walk and is returned; the stream is then the caller's to drain.
template <class F>
int for_each_band(dsh_ctx *c, const BandQuery &q, F &&per_band)
{
    const uint64_t band_floats = std::max<uint64_t>(c->threshold_band_bytes / sizeof(float), 1);
    const uint64_t ncols = q.rect && q.ce > q.cb ? q.ce - q.cb : 0;
    for (uint64_t b0 = q.rb, b1; b0 < q.re; b0 = b1) {
        b1 = q.rect ? std::min<uint64_t>(q.re, b0 + plan::rect_band_rows(ncols, band_floats))
                    : plan::tri_band_end(c->n, b0, q.re, band_floats, q.row_cap);
        const uint64_t span = q.rect ? (b1 - b0) * ncols : dsh_tri_span(c->n, b0, b1);
        if (!span && !q.empty_bands) continue;
        ThrRows g;
        int rc = thr_geometry(c, q.rect, c->n, b0, b1, ncols, q.cb, g);
        if (rc || (rc = compute_band(c, q.estim, q.result_type, q.k, g, span)) || (rc = per_band(g, (const float *)c->thr_vals.ptr, span)))
            return rc;
    }
    return DSH_OK;
}

// where the values of a walk over the whole triangle come from: the resident sketches, or a caller's packed triangle of n
// nodes on the host (dsh_mst_tri, dsh_dbscan_tri)
struct BandSource {
    const float *tri = nullptr;
    int estim = 0, result_type = 0, k = 0;
};

// the band walk over either source: the caller's triangle is cut by the same rule and uploaded band by band into c->thr_vals
template <class F>
int for_each_source_band(dsh_ctx *c, uint64_t n, const BandSource &s, F &&per_band)
{
    if (!s.tri) {
        BandQuery bq;
        bq.estim = s.estim, bq.result_type = s.result_type, bq.k = s.k;
        bq.re = n;
        return for_each_band(c, bq, per_band);
    }
    const uint64_t band_floats = std::max<uint64_t>(c->threshold_band_bytes / sizeof(float), 1);
    for (uint64_t b0 = 0, b1; b0 < n; b0 = b1) {
        b1 = plan::tri_band_end(n, b0, n, band_floats, kBandMaxRows);
        const uint64_t span = dsh_tri_span(n, b0, b1);
        if (!span) continue;
        ThrRows g;
        int rc = thr_geometry(c, 0, n, b0, b1, 0, 0, g);
        if (rc) return rc;
        HIPCHK(c, c->thr_vals.ensure(span * sizeof(float)));
        HIPCHK(c, hipMemcpyAsync(c->thr_vals.ptr, s.tri + dsh_tri_span(n, 0, b0), span * sizeof(float), hipMemcpyHostToDevice, c->stream));
        if ((rc = per_band(g, (const float *)c->thr_vals.ptr, span))) return rc;
    }
    return DSH_OK;
}

}  // namespace dsh
