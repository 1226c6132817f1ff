// greedy.hip -- dsh_greedy_threshold*: greedy representatives at a threshold, in slot order, on the device (DESIGN.md
// 4.11).  The band walk of bands.h -- the band buffer of dsh_dist_threshold*, the dense path unchanged -- with one more
// cap on a band's rows (BandQuery::row_cap = the option greedy_band_rows) and, per band,
// k_greedy_diag (the band's rows among themselves, sequential, in LDS) then k_greedy_band (its representative rows against
// every later column) in the place of k_cc_band (kernels_greedy.hip).  No host wait between bands; one wait at the end
// reads the count.  There is no give-up path: no loop of the kernels depends on another thread.
#include <algorithm>

#include "bands.h"

using namespace dsh;

namespace {

int greedy_bands(dsh_ctx *c, int estim, int result_type, int k, float t, uint32_t *d_labels, uint32_t *h_labels, uint64_t *n_reps)
{
    const uint64_t n = c->n;
    const int descending = measure_descending(result_type) ? 1 : 0;
    HIPCHK(c, c->gr.assign.ensure(n * sizeof(uint32_t)));
    HIPCHK(c, c->gr.state.ensure(sizeof(uint64_t)));
    if (!d_labels) {
        HIPCHK(c, c->gr.labels.ensure(n * sizeof(uint32_t)));
        d_labels = (uint32_t *)c->gr.labels.ptr;
    }
    uint32_t *assign = (uint32_t *)c->gr.assign.ptr;
    uint64_t *d_reps = (uint64_t *)c->gr.state.ptr;
    HIPCHK(c, hipMemsetAsync(d_reps, 0, sizeof(uint64_t), c->stream));
    HIPCHK(c, launch_cc_init(c->stream, assign, n));  // assign[x] = x
    BandQuery bq;
    bq.estim = estim, bq.result_type = result_type, bq.k = k;
    bq.re = n;
    bq.row_cap = c->gr.band_rows;
    const int rc = for_each_band(c, bq, [&](const ThrRows &g, const float *vals, uint64_t) -> int {
        hipError_t e = launch_greedy_diag(c->stream, vals, g, t, descending, assign);
        if (e == hipSuccess) e = launch_greedy_band(c->stream, vals, g, t, descending, assign);
        return e == hipSuccess ? DSH_OK : fail(c, DSH_EIO, "k_greedy_diag/k_greedy_band: %s", hipGetErrorString(e));
    });
    if (rc) return rc;
    HIPCHK(c, launch_greedy_labels(c->stream, assign, n, d_labels, d_reps));
    uint64_t reps = 0;
    HIPCHK(c, hipMemcpyAsync(&reps, d_reps, sizeof reps, hipMemcpyDeviceToHost, c->stream));
    if (h_labels) HIPCHK(c, hipMemcpyAsync(h_labels, d_labels, n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_reps) *n_reps = reps;
    return DSH_OK;
}

// d_labels: the caller's device buffer, or nullptr for h_labels (host)
int run_greedy_threshold(dsh_ctx *c, int estim, int result_type, int k, float t, uint32_t *d_labels, uint32_t *h_labels, uint64_t *n_reps)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    if (c->n && !d_labels && !h_labels) return DSH_EINVAL;
    if (c->n > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "%llu sketches: labels are 32-bit", (unsigned long long)c->n);
    if (n_reps) *n_reps = 0;
    if (!c->n) return DSH_OK;
    if ((rc = greedy_bands(c, estim, result_type, k, t, d_labels, h_labels, n_reps))) return drain(c, rc);
    return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_greedy_threshold(dsh_ctx *c, int estim, int result_type, int k, float threshold, uint32_t *labels_out, uint64_t *n_reps)
{
    return run_greedy_threshold(c, estim, result_type, k, threshold, nullptr, labels_out, n_reps);
}

int dsh_greedy_threshold_device(dsh_ctx *c, int estim, int result_type, int k, float threshold, void *d_labels, uint64_t *n_reps)
{
    return run_greedy_threshold(c, estim, result_type, k, threshold, (uint32_t *)d_labels, nullptr, n_reps);
}

}  // extern "C"
