// group_stats.hip -- dsh_group_stats*: per-group statistics and medoids of a labelling.  Two routes to the
// same integer accumulators (kernels_group.hip), so to the same bytes:
//   dense   the band walk of bands.h -- the band rule and the band buffer of dsh_dist_threshold* -- with k_gs_rows and
//           k_gs_cols per band;
//   pairs   the intra-group pairs enumerated on the device chunk by chunk from the member CSR (k_gs_enum, lhs = the larger
//           slot: the triangle's bits) and computed by the direct pair path of pairs.hip (pairs_ensure_cards +
//           pairs_run_chunk), each chunk folded into both ends by k_gs_pairs.  Nothing of the size of P_in exists at once.
// Then k_gs_medoid / k_gs_finish.  No host wait between bands or chunks; one wait at the end.
#include <algorithm>
#include <vector>

#include "bands.h"

using namespace dsh;

namespace {

// auto route: pairs iff kGsPairsDivisor * P_in <= n (n - 1) / 2 -- the 5 % break-even of pair lists against the dense path at
// p = 14 (profiles/pairs1); this call's own crossover: 4.1 % at 10 000 x p=14, 5.7 % at 100 000 x p=10 (profiles/stats1)
constexpr uint64_t kGsPairsDivisor = 20;

struct GsOut {  // device pointers; a null one is not written
    uint32_t *medoid, *cnt;
    int64_t *sum;
    float *worst;
};

int gs_dense(dsh_ctx *c, int estim, int result_type, int k, const uint32_t *d_labels, const GsAccum &acc)
{
    const int descending = measure_descending(result_type) ? 1 : 0;
    BandQuery bq;
    bq.estim = estim, bq.result_type = result_type, bq.k = k;
    bq.re = c->n;
    return for_each_band(c, bq, [&](const ThrRows &g, const float *vals, uint64_t) -> int {
        hipError_t e = launch_gs_rows(c->stream, vals, g, d_labels, descending, acc);
        if (e == hipSuccess) e = launch_gs_cols(c->stream, vals, g, d_labels, descending, acc);
        return e == hipSuccess ? DSH_OK : fail(c, DSH_EIO, "k_gs_rows/k_gs_cols: %s", hipGetErrorString(e));
    });
}

// the groups of at least two members, in label order, their members in slot order (a counting sort)
struct GsCsr {
    std::vector<uint64_t> ppre;
    std::vector<uint32_t> moff, mem;
};

void gs_build_csr(const uint32_t *labels, uint64_t n, const std::vector<uint32_t> &size, GsCsr &s)
{
    std::vector<uint32_t> at(n, 0xFFFFFFFFu);  // per label: where its next member goes
    s.ppre.assign(1, 0);
    s.moff.assign(1, 0);
    for (uint64_t l = 0; l < n; ++l) {
        const uint64_t sz = size[l];
        if (sz < 2) continue;
        at[l] = s.moff.back();
        s.ppre.push_back(s.ppre.back() + sz * (sz - 1) / 2);
        s.moff.push_back((uint32_t)(s.moff.back() + sz));
    }
    s.mem.resize(s.moff.back());
    for (uint64_t x = 0; x < n; ++x)
        if (at[labels[x]] != 0xFFFFFFFFu) s.mem[at[labels[x]]++] = (uint32_t)x;
}

int gs_pairs(dsh_ctx *c, int estim, int result_type, int k, uint64_t p_in, const GsCsr &s, const GsAccum &acc)
{
    if (!p_in) return DSH_OK;
    PairsQuery q;
    q.estim = estim, q.k = k, q.n_types = 1;
    for (uint32_t t = 0; t < 9; ++t) q.types.t[t] = 0;
    q.types.t[0] = result_type;
    const int descending = measure_descending(result_type) ? 1 : 0;
    const uint64_t ng = s.ppre.size() - 1;
    const size_t pb = (ng + 1) * sizeof(uint64_t), ob = (ng + 1) * sizeof(uint32_t), mb = s.mem.size() * sizeof(uint32_t);
    HIPCHK(c, c->gs.csr.ensure(pb + ob + mb));
    char *base = (char *)c->gs.csr.ptr;
    HIPCHK(c, hipMemcpyAsync(base, s.ppre.data(), pb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(base + pb, s.moff.data(), ob, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(base + pb + ob, s.mem.data(), mb, hipMemcpyHostToDevice, c->stream));
    const uint64_t chunk = std::min<uint64_t>(c->pairs.chunk, p_in);
    HIPCHK(c, c->pairs.lhs.ensure(chunk * sizeof(uint32_t)));
    HIPCHK(c, c->pairs.rhs.ensure(chunk * sizeof(uint32_t)));
    HIPCHK(c, c->pairs.out.ensure(chunk * sizeof(float)));
    int rc = pairs_ensure_cards(c, estim);
    if (rc) return rc;
    uint32_t *lhs = (uint32_t *)c->pairs.lhs.ptr, *rhs = (uint32_t *)c->pairs.rhs.ptr;
    float *vals = (float *)c->pairs.out.ptr;
    for (uint64_t x0 = 0; x0 < p_in; x0 += chunk) {
        const uint64_t cnt = std::min<uint64_t>(chunk, p_in - x0);
        HIPCHK(c, launch_gs_enum(c->stream, (const uint64_t *)base, (const uint32_t *)(base + pb), (const uint32_t *)(base + pb + ob), ng, x0,
                                 cnt, lhs, rhs));
        if ((rc = pairs_run_chunk(c, q, lhs, rhs, x0, cnt, vals, chunk))) return rc;
        HIPCHK(c, launch_gs_pairs(c->stream, lhs, rhs, vals, cnt, c->n, descending, acc));
    }
    return DSH_OK;
}

int run_group_stats(dsh_ctx *c, int estim, int result_type, int k, const uint32_t *labels, bool device, uint32_t *medoid_out,
                    uint32_t *cnt_out, int64_t *sum_out, float *worst_out)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    const uint64_t n = c->n;
    if (n > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "%llu sketches: labels are 32-bit", (unsigned long long)n);
    if (estim < 0 || estim > 2) return fail(c, DSH_EINVAL, "bad estimator %d", estim);
    if (result_type == DSH_SIZES) return fail(c, DSH_EINVAL, "DSH_SIZES has no statistics: its values are set sizes, not in (-2, 2)");
    if (result_type < 0 || result_type > 8) return fail(c, DSH_EINVAL, "unsupported result_type %d", result_type);
    if (n && !labels) return fail(c, DSH_EINVAL, "no labels for %llu sketches", (unsigned long long)n);
    for (uint64_t x = 0; x < n; ++x)
        if (labels[x] >= n)
            return fail(c, DSH_EINVAL, "labels[%llu] = %u outside [0, %llu)", (unsigned long long)x, labels[x], (unsigned long long)n);
    if (!n) return DSH_OK;
    // P_in, the route
    std::vector<uint32_t> size(n, 0);
    for (uint64_t x = 0; x < n; ++x) ++size[labels[x]];
    uint64_t p_in = 0;
    for (uint64_t l = 0; l < n; ++l) p_in += (uint64_t)size[l] * (size[l] ? size[l] - 1 : 0) / 2;
    const uint64_t tri = n * (n - 1) / 2;
    const int route = c->gs.route >= 0 ? c->gs.route : (p_in <= tri / kGsPairsDivisor ? 1 : 0);  // 20 P_in <= n (n - 1) / 2
    if (route == 1 && p_in && k < 1) return fail(c, DSH_EINVAL, "bad k %d", k);
    c->gs.route_last = route;
    GsCsr csr;  // (uploaded from where it stands: it lives until the call's wait)
    if (route == 1 && p_in) gs_build_csr(labels, n, size, csr);

    // accumulators: sum[n] | cnt[n] | wkey[n], zero; groups: g_sum[n] | g_cnt[n] zero, g_slot[n] all ones
    HIPCHK(c, c->gs.labels.ensure(n * sizeof(uint32_t)));
    HIPCHK(c, c->gs.acc.ensure(n * 16));
    HIPCHK(c, c->gs.grp.ensure(n * 16));
    GsAccum acc;
    acc.sum = (uint64_t *)c->gs.acc.ptr;
    acc.cnt = (uint32_t *)(acc.sum + n);
    acc.wkey = acc.cnt + n;
    uint64_t *g_sum = (uint64_t *)c->gs.grp.ptr;
    uint32_t *g_cnt = (uint32_t *)(g_sum + n), *g_slot = g_cnt + n;
    uint32_t *d_labels = (uint32_t *)c->gs.labels.ptr;
    GsOut o = {medoid_out, cnt_out, sum_out, worst_out};
    if (!device) {  // the host form's outputs pass through the library's own buffer: sum[n] | medoid[n] | cnt[n] | worst[n]
        HIPCHK(c, c->gs.out.ensure(n * 20));
        o.sum = sum_out ? (int64_t *)c->gs.out.ptr : nullptr;
        o.medoid = medoid_out ? (uint32_t *)((int64_t *)c->gs.out.ptr + n) : nullptr;
        o.cnt = cnt_out ? (uint32_t *)((int64_t *)c->gs.out.ptr + n) + n : nullptr;
        o.worst = worst_out ? (float *)((int64_t *)c->gs.out.ptr + n) + 2 * n : nullptr;
    }
    HIPCHK(c, hipMemcpyAsync(d_labels, labels, n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemsetAsync(c->gs.acc.ptr, 0, n * 16, c->stream));
    HIPCHK(c, hipMemsetAsync(c->gs.grp.ptr, 0, n * 12, c->stream));
    HIPCHK(c, hipMemsetAsync(g_slot, 0xFF, n * sizeof(uint32_t), c->stream));
    if (route == 1 && p_in && (rc = pairs_err_begin(c))) return drain(c, rc);
    rc = route == 1 ? gs_pairs(c, estim, result_type, k, p_in, csr, acc) : gs_dense(c, estim, result_type, k, d_labels, acc);
    if (rc) return drain(c, rc);
    const int descending = measure_descending(result_type) ? 1 : 0;
    const hipError_t e = launch_gs_finish(c->stream, d_labels, n, descending, acc, g_cnt, g_sum, g_slot, o.medoid, o.cnt, o.sum, o.worst);
    if (e != hipSuccess) return drain(c, fail(c, DSH_EIO, "k_gs_medoid/k_gs_finish: %s", hipGetErrorString(e)));
    if (!device) {
        hipError_t h = hipSuccess;
        if (medoid_out) h = hipMemcpyAsync(medoid_out, o.medoid, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
        if (h == hipSuccess && cnt_out) h = hipMemcpyAsync(cnt_out, o.cnt, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
        if (h == hipSuccess && sum_out) h = hipMemcpyAsync(sum_out, o.sum, n * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
        if (h == hipSuccess && worst_out) h = hipMemcpyAsync(worst_out, o.worst, n * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (h != hipSuccess) return drain(c, fail(c, DSH_EIO, "copy of the statistics failed: %s", hipGetErrorString(h)));
    }
    if (route == 1 && p_in) {  // the one wait, with the pair path's error words
        if ((rc = pairs_err_end(c))) return drain(c, rc);
        return DSH_OK;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_group_stats(dsh_ctx *c, int estim, int result_type, int k, const uint32_t *labels, uint32_t *medoid_out, uint32_t *cnt_out,
                    int64_t *sum_out, float *worst_out)
{
    return run_group_stats(c, estim, result_type, k, labels, false, medoid_out, cnt_out, sum_out, worst_out);
}

int dsh_group_stats_device(dsh_ctx *c, int estim, int result_type, int k, const uint32_t *labels, void *d_medoid, void *d_cnt, void *d_sum,
                           void *d_worst)
{
    return run_group_stats(c, estim, result_type, k, labels, true, (uint32_t *)d_medoid, (uint32_t *)d_cnt, (int64_t *)d_sum,
                           (float *)d_worst);
}

}  // extern "C"
