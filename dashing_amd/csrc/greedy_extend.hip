// greedy_extend.hip -- dsh_greedy_extend*: the greedy representatives of dsh_greedy_threshold* continued behind a labelling
// the caller brings (slots [0, m) keep their labels, slots [m, n) are judged), with the covered slots given to the FIRST
// or to the BEST representative that hits them.  Two phases on the ctx stream, the dense path unchanged:
//   1. the old representatives against the new columns: bands of old rows (plan::greedy_old_band: from a representative to
//      a representative, stretches without one skipped), each computed into the library-owned band buffer (bands.h:
//      thr_geometry + compute_band) and walked by k_greedy_rect;
//   2. the new rows among themselves: the band walk of greedy.hip (bands.h) started at row m -- k_greedy_diag, then k_greedy_band
//      (FIRST) or k_greedy_best (BEST), kernels_greedy.hip.
// k_greedy_extend_labels writes the labels.  No host wait between bands; one wait at the end reads the count.
#include <algorithm>

#include "bands.h"

using namespace dsh;

namespace {

int extend_bands(dsh_ctx *c, int estim, int result_type, int k, float t, int best_mode, uint64_t m, const uint32_t *labels_in,
                 uint32_t *d_labels, uint32_t *h_labels, uint64_t *n_reps)
{
    const uint64_t n = c->n;
    const int descending = measure_descending(result_type) ? 1 : 0;
    const uint64_t band_floats = std::max<uint64_t>(c->threshold_band_bytes / sizeof(float), 1);
    HIPCHK(c, c->gr.assign.ensure(n * sizeof(uint32_t)));
    HIPCHK(c, c->gr.state.ensure(sizeof(uint64_t)));
    if (best_mode) HIPCHK(c, c->gr.best.ensure(std::max<uint64_t>(n - m, 1) * sizeof(uint64_t)));
    if (!d_labels) {
        HIPCHK(c, c->gr.labels.ensure(n * sizeof(uint32_t)));
        d_labels = (uint32_t *)c->gr.labels.ptr;
    }
    uint32_t *assign = (uint32_t *)c->gr.assign.ptr;
    uint64_t *best = best_mode ? (uint64_t *)c->gr.best.ptr : nullptr;
    uint64_t *d_reps = (uint64_t *)c->gr.state.ptr;
    HIPCHK(c, hipMemsetAsync(d_reps, 0, sizeof(uint64_t), c->stream));
    HIPCHK(c, launch_cc_init(c->stream, assign, n));  // assign[x] = x
    if (m) HIPCHK(c, hipMemcpyAsync(assign, labels_in, m * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (best && n > m) HIPCHK(c, hipMemsetAsync(best, 0, (n - m) * sizeof(uint64_t), c->stream));
    // phase 1: old representatives x new columns
    if (m && m < n) {
        const uint64_t ncols = n - m;
        uint64_t b0 = 0, b1 = 0;
        for (uint64_t from = 0; plan::greedy_old_band(labels_in, m, ncols, from, band_floats, b0, b1); from = b1) {
            ThrRows g;
            int rc = thr_geometry(c, 1, n, b0, b1, ncols, m, g);
            if (rc || (rc = compute_band(c, estim, result_type, k, g, g.rows * ncols))) return rc;
            const hipError_t e = launch_greedy_rect(c->stream, (const float *)c->thr_vals.ptr, g, t, descending, assign, best);
            if (e != hipSuccess) return fail(c, DSH_EIO, "k_greedy_rect: %s", hipGetErrorString(e));
        }
    }
    // phase 2: the new rows among themselves (a column an old representative covered is simply "not itself")
    BandQuery bq;
    bq.estim = estim, bq.result_type = result_type, bq.k = k;
    bq.rb = m, bq.re = n;
    bq.row_cap = c->gr.band_rows;
    const int rc = for_each_band(c, bq, [&](const ThrRows &g, const float *vals, uint64_t) -> int {
        hipError_t e = launch_greedy_diag(c->stream, vals, g, t, descending, assign);
        if (e == hipSuccess)
            e = best ? launch_greedy_best(c->stream, vals, g, t, descending, assign, best, m) : launch_greedy_band(c->stream, vals, g, t, descending, assign);
        return e == hipSuccess ? DSH_OK : fail(c, DSH_EIO, "k_greedy_diag/k_greedy_band/k_greedy_best: %s", hipGetErrorString(e));
    });
    if (rc) return rc;
    HIPCHK(c, launch_greedy_extend_labels(c->stream, assign, best, m, n, d_labels, d_reps));
    uint64_t reps = 0;
    HIPCHK(c, hipMemcpyAsync(&reps, d_reps, sizeof reps, hipMemcpyDeviceToHost, c->stream));
    if (h_labels) HIPCHK(c, hipMemcpyAsync(h_labels, d_labels, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_reps) *n_reps = reps;
    return DSH_OK;
}

// d_labels: the caller's device buffer, or nullptr for h_labels (host)
int run_greedy_extend(dsh_ctx *c, int estim, int result_type, int k, float t, int assign_mode, uint64_t m, const uint32_t *labels_in,
                      uint32_t *d_labels, uint32_t *h_labels, uint64_t *n_reps)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    const uint64_t n = c->n;
    if (n && !d_labels && !h_labels) return fail(c, DSH_EINVAL, "no output for %llu labels", (unsigned long long)n);
    if (n > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "%llu sketches: labels are 32-bit", (unsigned long long)n);
    if (assign_mode != DSH_GREEDY_FIRST && assign_mode != DSH_GREEDY_BEST) return fail(c, DSH_EINVAL, "assign_mode %d is neither DSH_GREEDY_FIRST nor DSH_GREEDY_BEST", assign_mode);
    if (m > n) return fail(c, DSH_EINVAL, "first_new %llu is beyond the %llu sketches", (unsigned long long)m, (unsigned long long)n);
    if ((labels_in == nullptr) != (m == 0)) return fail(c, DSH_EINVAL, "labels_in is NULL if and only if first_new is 0");
    for (uint64_t x = 0; x < m; ++x) {
        const uint32_t l = labels_in[x];
        if (l > x) return fail(c, DSH_EINVAL, "labels_in[%llu] = %u is behind its slot", (unsigned long long)x, l);
        if (labels_in[l] != l) return fail(c, DSH_EINVAL, "labels_in[%llu] = %u is not a representative (labels_in[%u] = %u)", (unsigned long long)x, l, l, labels_in[l]);
    }
    if (n_reps) *n_reps = 0;
    if (!n) return DSH_OK;
    if ((rc = extend_bands(c, estim, result_type, k, t, assign_mode == DSH_GREEDY_BEST, m, labels_in, d_labels, h_labels, n_reps)))
        return drain(c, rc);
    return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_greedy_extend(dsh_ctx *c, int estim, int result_type, int k, float threshold, int assign_mode, uint64_t first_new,
                      const uint32_t *labels_in, uint32_t *labels_out, uint64_t *n_reps)
{
    return run_greedy_extend(c, estim, result_type, k, threshold, assign_mode, first_new, labels_in, nullptr, labels_out, n_reps);
}

int dsh_greedy_extend_device(dsh_ctx *c, int estim, int result_type, int k, float threshold, int assign_mode, uint64_t first_new,
                             const uint32_t *labels_in, void *d_labels, uint64_t *n_reps)
{
    return run_greedy_extend(c, estim, result_type, k, threshold, assign_mode, first_new, labels_in, (uint32_t *)d_labels, nullptr, n_reps);
}

}  // extern "C"
