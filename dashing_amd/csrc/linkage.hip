// linkage.hip -- dsh_linkage_threshold*, dsh_linkage_tri: single-, complete- and average-linkage clusters at a threshold
// (include/dashing_hip.h has the contract, linkage.h the step logic, kernels_linkage.hip the kernels).
//   1. partition   every merge needs a passing member pair, so the components of the graph of passing pairs split the problem:
//                  the union-find of dsh_cluster_threshold (cluster.hip) over the band walk, at the threshold itself or, for
//                  AVERAGE, at the loose float threshold of the quantised graph (lk_loose_threshold).  Its labels come to the
//                  host: the first of the call's two waits
//   2. tables      the components of at least two members as a member CSR, cut into batches whose cell matrices fit
//                  "linkage_budget_bytes"; one component beyond the budget fails the call with DSH_ENOMEM before anything else
//                  is enqueued
//   3. per batch   fill -- dense: the band walk again with k_lk_fill_band; pairs: the intra-component pairs enumerated chunk by
//                  chunk (k_gs_enum), computed by the direct pair path (pairs_run_chunk) and scattered by k_lk_fill_pairs --
//                  then k_linkage, one workgroup per component
//   4. the labels go out (k_greedy_labels copies and counts them); the second wait reads the count and the error word
// dsh_linkage_tri runs the same over a caller's triangle, which travels through the band buffer band by band.
#include <algorithm>
#include <cmath>
#include <functional>
#include <vector>

#include "bands.h"
#include "linkage.h"

using namespace dsh;

namespace {

constexpr uint64_t kLkPairsDivisor = 20;  // auto route: pairs iff 20 P_in <= n (n - 1) / 2, the rule of dsh_group_stats

struct LkState {  // lk_state on the device (what launch_greedy_labels counts into, and the error word)
    unsigned long long n_roots;
    uint32_t err, pad_;
};

// where the values come from: the resident sketches, or a caller's triangle on the host
struct LkSource {
    const float *tri = nullptr;
    int estim = 0, result_type = 0, k = 0;
};

typedef std::function<int(const ThrRows &, const float *, uint64_t)> PerBand;

// the band walk of bands.h over either source
int lk_walk(dsh_ctx *c, uint64_t n, const LkSource &s, const PerBand &per_band)
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

// n singletons, or whatever labels the device holds: out to the caller, counted; the call's last wait
int lk_finish(dsh_ctx *c, uint64_t n, bool pairs_route, uint32_t *d_labels, uint32_t *h_labels, uint64_t *n_clusters)
{
    LkState *st = (LkState *)c->lk.state.ptr;
    uint32_t *out = d_labels;
    if (!out) {
        HIPCHK(c, c->cc.labels.ensure(std::max<uint64_t>(n, 1) * sizeof(uint32_t)));
        out = (uint32_t *)c->cc.labels.ptr;
    }
    HIPCHK(c, launch_greedy_labels(c->stream, (const uint32_t *)c->lk.labels.ptr, n, out, (uint64_t *)&st->n_roots));
    LkState h = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(&h, st, sizeof h, hipMemcpyDeviceToHost, c->stream));
    if (h_labels) HIPCHK(c, hipMemcpyAsync(h_labels, out, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (pairs_route) {  // the wait, with the pair path's error words
        const int rc = pairs_err_end(c);
        if (rc) return rc;
    } else {
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (h.err) return fail(c, DSH_EIO, "internal: linkage step bound exceeded (code %u)", h.err);
    if (n_clusters) *n_clusters = h.n_roots;
    return DSH_OK;
}

int lk_begin(dsh_ctx *c, uint64_t n)
{
    HIPCHK(c, c->lk.labels.ensure(std::max<uint64_t>(n, 1) * sizeof(uint32_t)));
    HIPCHK(c, c->lk.state.ensure(sizeof(LkState)));
    HIPCHK(c, hipMemsetAsync(c->lk.state.ptr, 0, sizeof(LkState), c->stream));
    HIPCHK(c, launch_cc_init(c->stream, (uint32_t *)c->lk.labels.ptr, n));
    return DSH_OK;
}

// the checks of the linkage and the threshold that both forms share (result_type < 0: a caller's triangle)
int lk_check(dsh_ctx *c, int linkage, float t)
{
    if (linkage < kLkSingle || linkage > kLkAverage) return fail(c, DSH_EINVAL, "unknown linkage %d", linkage);
    if (linkage == kLkAverage && t == t && !(std::fabs(t) < 2.f))
        return fail(c, DSH_EINVAL, "average linkage judges values in (-2, 2): threshold %g", (double)t);
    return DSH_OK;
}

int run_linkage(dsh_ctx *c, uint64_t n, const LkSource &src, int descending, float t, int linkage, uint32_t *d_labels, uint32_t *h_labels,
                uint64_t *n_clusters)
{
    int rc;
    if (n < 2 || t != t) {  // nothing to merge; a NaN threshold passes nothing
        if ((rc = lk_begin(c, n)) || (rc = lk_finish(c, n, false, d_labels, h_labels, n_clusters))) return drain(c, rc);
        return DSH_OK;
    }
    // 1. the components of the graph of passing pairs
    std::vector<uint32_t> lab(n, 0);
    if (c->lk.partition) {
        const float loose = linkage == kLkAverage ? lk_loose_threshold(t, descending) : t;
        if ((rc = cc_begin(c, n))) return drain(c, rc);
        rc = lk_walk(c, n, src, [&](const ThrRows &g, const float *vals, uint64_t) -> int {
            const hipError_t e = launch_cc_band(c->stream, vals, g, loose, descending, (uint32_t *)c->cc.parent.ptr, cc_cap(n), cc_err(c));
            return e == hipSuccess ? DSH_OK : fail(c, DSH_EIO, "k_cc_band: %s", hipGetErrorString(e));
        });
        if (rc || (rc = cc_finish(c, n, nullptr, lab.data(), nullptr))) return drain(c, rc);
    }
    // 2. the tables: components of at least two members in label order, members in slot order
    std::vector<uint32_t> comp(n, kLkNone), rank(n, 0), moff(1, 0), mem;
    {
        std::vector<uint32_t> size(n, 0), of_label(n, kLkNone), at(n, 0);  // per label: members, component, where its next member goes
        for (uint64_t x = 0; x < n; ++x) {
            if (lab[x] >= n) return fail(c, DSH_EIO, "internal: component label %u of slot %llu", lab[x], (unsigned long long)x);
            ++size[lab[x]];
        }
        for (uint64_t l = 0; l < n; ++l) {
            if (size[l] < 2) continue;
            of_label[l] = (uint32_t)(moff.size() - 1);
            at[l] = moff.back();
            moff.push_back(moff.back() + size[l]);
        }
        mem.resize(moff.back());
        for (uint64_t x = 0; x < n; ++x) {
            const uint32_t l = lab[x], ci = of_label[l];
            if (ci == kLkNone) continue;
            comp[x] = ci;
            rank[x] = at[l] - moff[ci];
            mem[at[l]++] = (uint32_t)x;
        }
    }
    const uint64_t ncomp = moff.size() - 1;
    const uint64_t cellsz = linkage == kLkAverage ? 8 : 4;
    std::vector<uint64_t> coff(ncomp, 0), ppre(ncomp + 1, 0);
    std::vector<uint32_t> batch(1, 0);  // first component of every batch, and the end
    uint64_t max_cells = 0, max_members = 0, max_m = 0;
    {
        uint64_t cells = 0;
        for (uint64_t ci = 0; ci < ncomp; ++ci) {
            const uint64_t m = moff[ci + 1] - moff[ci], need = m * m * cellsz;
            ppre[ci + 1] = ppre[ci] + m * (m - 1) / 2;
            if (linkage == kLkAverage && m > kLkAvgMaxMembers)
                return fail(c, DSH_ENOMEM, "a component of m = %llu members: average linkage takes at most %u (64-bit sums), and its matrix would need %llu bytes",
                            (unsigned long long)m, kLkAvgMaxMembers, (unsigned long long)need);
            if (m > (1ull << 30) || need > c->lk.budget)  // (m <= 2^30: need did not wrap)
                return fail(c, DSH_ENOMEM, "a component of m = %llu members needs a matrix of %llu bytes, linkage_budget_bytes is %llu",
                            (unsigned long long)m, (unsigned long long)need, (unsigned long long)c->lk.budget);
            if (cells && (cells + m * m) * cellsz > c->lk.budget) {
                batch.push_back((uint32_t)ci);
                cells = 0;
            }
            coff[ci] = cells;
            cells += m * m;
            max_cells = std::max(max_cells, cells);
            max_members = std::max<uint64_t>(max_members, moff[ci + 1] - moff[batch.back()]);
            max_m = std::max(max_m, m);
        }
        batch.push_back((uint32_t)ncomp);
    }
    const uint64_t p_in = ppre[ncomp], tri_pairs = n * (n - 1) / 2;
    const int route = src.tri ? 0 : (c->lk.route >= 0 ? c->lk.route : (p_in <= tri_pairs / kLkPairsDivisor ? 1 : 0));
    if (!src.tri) c->lk.route_last = route;
    const bool pairs = route == 1 && p_in;
    if (pairs && src.k < 1) return fail(c, DSH_EINVAL, "bad k %d", src.k);
    if ((rc = lk_begin(c, n))) return drain(c, rc);
    if (!ncomp) {
        if ((rc = lk_finish(c, n, false, d_labels, h_labels, n_clusters))) return drain(c, rc);
        return DSH_OK;
    }
    // the tables on the device: ppre | coff | comp | rank | moff | mem (8-byte entries first)
    const size_t b_ppre = (ncomp + 1) * 8, b_coff = ncomp * 8, b_n = n * 4, b_moff = (ncomp + 1) * 4, b_mem = mem.size() * 4;
    HIPCHK(c, c->lk.tab.ensure(b_ppre + b_coff + 2 * b_n + b_moff + b_mem));
    char *tab = (char *)c->lk.tab.ptr;
    const uint64_t *d_ppre = (const uint64_t *)tab;
    LkComps C;
    C.coff = (const uint64_t *)(tab + b_ppre);
    C.comp = (const uint32_t *)(tab + b_ppre + b_coff);
    C.rank = C.comp + n;
    C.moff = C.rank + n;
    C.mem = C.moff + ncomp + 1;
    if (hipMemcpyAsync((void *)d_ppre, ppre.data(), b_ppre, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync((void *)C.coff, coff.data(), b_coff, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync((void *)C.comp, comp.data(), b_n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync((void *)C.rank, rank.data(), b_n, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync((void *)C.moff, moff.data(), b_moff, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
        hipMemcpyAsync((void *)C.mem, mem.data(), b_mem, hipMemcpyHostToDevice, c->stream) != hipSuccess)
        return drain(c, fail(c, DSH_EIO, "upload of the components' tables failed"));
    {
        const hipError_t e1 = c->lk.cells.ensure(max_cells * cellsz), e2 = c->lk.nodes.ensure(max_members * (cellsz + 16));
        if (e1 != hipSuccess || e2 != hipSuccess) {
            (void)hipGetLastError();
            return drain(c, fail(c, DSH_ENOMEM, "no device memory for the matrices of a batch (%llu bytes)", (unsigned long long)(max_cells * cellsz)));
        }
    }
    PairsQuery pq;
    uint64_t chunk = 0;
    if (pairs) {
        pq.estim = src.estim, pq.k = src.k, pq.n_types = 1;
        for (uint32_t x = 0; x < 9; ++x) pq.types.t[x] = 0;
        pq.types.t[0] = src.result_type;
        chunk = std::min<uint64_t>(c->pairs.chunk, p_in);
        HIPCHK(c, c->pairs.lhs.ensure(chunk * sizeof(uint32_t)));
        HIPCHK(c, c->pairs.rhs.ensure(chunk * sizeof(uint32_t)));
        HIPCHK(c, c->pairs.out.ensure(chunk * sizeof(float)));
        if ((rc = pairs_ensure_cards(c, src.estim)) || (rc = pairs_err_begin(c))) return drain(c, rc);
    }
    // 3. batch by batch
    const uint32_t cap = (uint32_t)std::min<uint64_t>(max_m + 1, 0xFFFFFFFFull);
    uint32_t *err = &((LkState *)c->lk.state.ptr)->err;
    for (size_t q = 0; q + 1 < batch.size(); ++q) {
        LkBatch B;
        B.c0 = batch[q], B.c1 = batch[q + 1];
        B.cells = c->lk.cells.ptr;
        B.ncells = c->lk.cells.cap / cellsz;
        B.state = c->lk.nodes.ptr;
        B.mbase = moff[B.c0];
        B.members = moff[B.c1] - moff[B.c0];
        uint32_t lds_members = 0;
        for (uint32_t ci = B.c0; ci < B.c1; ++ci) {
            const uint32_t m = moff[ci + 1] - moff[ci];
            if (m <= c->lk.lds_max) lds_members = std::max(lds_members, m);
        }
        if (pairs) {
            uint32_t *lhs = (uint32_t *)c->pairs.lhs.ptr, *rhs = (uint32_t *)c->pairs.rhs.ptr;
            float *vals = (float *)c->pairs.out.ptr;
            for (uint64_t x0 = ppre[B.c0]; x0 < ppre[B.c1]; x0 += chunk) {
                const uint64_t cnt = std::min<uint64_t>(chunk, ppre[B.c1] - x0);
                if (launch_gs_enum(c->stream, d_ppre, C.moff, C.mem, ncomp, x0, cnt, lhs, rhs) != hipSuccess)
                    return drain(c, fail(c, DSH_EIO, "k_gs_enum failed"));
                if ((rc = pairs_run_chunk(c, pq, lhs, rhs, x0, cnt, vals, chunk))) return drain(c, rc);
                if (launch_lk_fill_pairs(c->stream, linkage, lhs, rhs, vals, cnt, n, C, B, descending) != hipSuccess)
                    return drain(c, fail(c, DSH_EIO, "k_lk_fill_pairs failed"));
            }
        } else {
            rc = lk_walk(c, n, src, [&](const ThrRows &g, const float *vals, uint64_t) -> int {
                const hipError_t e = launch_lk_fill_band(c->stream, linkage, vals, g, C, B, descending);
                return e == hipSuccess ? DSH_OK : fail(c, DSH_EIO, "k_lk_fill_band: %s", hipGetErrorString(e));
            });
            if (rc) return drain(c, rc);
        }
        const hipError_t e = launch_linkage(c->stream, linkage, C, B, t, descending, c->lk.lds_max, lds_members, cap,
                                            (uint32_t *)c->lk.labels.ptr, err);
        if (e != hipSuccess) return drain(c, fail(c, DSH_EIO, "k_linkage: %s", hipGetErrorString(e)));
    }
    // 4. out
    if ((rc = lk_finish(c, n, pairs, d_labels, h_labels, n_clusters))) return drain(c, rc);
    return DSH_OK;
}

int run_linkage_threshold(dsh_ctx *c, int estim, int result_type, int k, float t, int linkage, uint32_t *d_labels, uint32_t *h_labels,
                          uint64_t *n_clusters)
{
    const uint64_t n = c->n;
    if (n > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "%llu sketches: labels are 32-bit", (unsigned long long)n);
    int rc = lk_check(c, linkage, t);
    if (rc) return rc;
    if (linkage == kLkAverage && result_type == DSH_SIZES)
        return fail(c, DSH_EINVAL, "DSH_SIZES has no average linkage: its values are set sizes, not in (-2, 2)");
    if (estim < 0 || estim > 2) return fail(c, DSH_EINVAL, "bad estimator %d", estim);
    if (result_type < 0 || result_type > 8) return fail(c, DSH_EINVAL, "unsupported result_type %d", result_type);
    if (n_clusters) *n_clusters = 0;
    if (!n) return DSH_OK;
    LkSource s;
    s.estim = estim, s.result_type = result_type, s.k = k;
    return run_linkage(c, n, s, measure_descending(result_type) ? 1 : 0, t, linkage, d_labels, h_labels, n_clusters);
}

}  // namespace

extern "C" {

int dsh_linkage_threshold(dsh_ctx *c, int estim, int result_type, int k, float threshold, int linkage, uint32_t *labels_out,
                          uint64_t *n_clusters)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    if (c->n && !labels_out) return DSH_EINVAL;
    return run_linkage_threshold(c, estim, result_type, k, threshold, linkage, nullptr, labels_out, n_clusters);
}

int dsh_linkage_threshold_device(dsh_ctx *c, int estim, int result_type, int k, float threshold, int linkage, void *d_labels,
                                 uint64_t *n_clusters)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    if (c->n && !d_labels) return DSH_EINVAL;
    return run_linkage_threshold(c, estim, result_type, k, threshold, linkage, (uint32_t *)d_labels, nullptr, n_clusters);
}

int dsh_linkage_tri(dsh_ctx *c, uint64_t n_nodes, const float *tri, int descending, float threshold, int linkage, uint32_t *labels_out,
                    uint64_t *n_clusters)
{
    if (!c) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    if (n_nodes > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "%llu nodes: labels are 32-bit (at most 2^32 - 1 nodes)", (unsigned long long)n_nodes);
    if ((rc = lk_check(c, linkage, threshold))) return rc;
    if (n_nodes && !labels_out) return DSH_EINVAL;
    if (n_nodes >= 2 && !tri) return fail(c, DSH_EINVAL, "no values for %llu nodes", (unsigned long long)n_nodes);
    if (n_clusters) *n_clusters = 0;
    if (!n_nodes) return DSH_OK;
    LkSource s;
    s.tri = n_nodes >= 2 ? tri : nullptr;
    if (n_nodes < 2) {  // (one node: no value is read)
        static const float none = 0.f;
        s.tri = &none;
    }
    return run_linkage(c, n_nodes, s, descending ? 1 : 0, threshold, linkage, nullptr, labels_out, n_clusters);
}

}  // extern "C"
