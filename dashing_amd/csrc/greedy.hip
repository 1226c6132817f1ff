// greedy.hip -- dsh_greedy_threshold*: greedy representatives at a threshold, in slot order, on the device (DESIGN.md
// 4.11).  The band loop of run_cluster_threshold (cluster.hip) -- PairJob::triangle + run_pairs into the library-owned band
// buffer, the dense path unchanged -- with one more cap on a band's rows (plan::greedy_band_end) and, per band,
// k_greedy_diag (the band's rows among themselves, sequential, in LDS) then k_greedy_band (its representative rows against
// every later column) in the place of k_cc_band (kernels_greedy.hip).  No host wait between bands; one wait at the end
// reads the count.  There is no give-up path: no loop of the kernels depends on another thread.
#include <algorithm>

#include "ctx.h"

using namespace dsh;

namespace {

// a failed enqueue: leave the stream idle, as every entry point does
int greedy_abort(dsh_ctx *c, int rc)
{
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    return rc;
}

int greedy_bands(dsh_ctx *c, int estim, int result_type, int k, float t, uint32_t *d_labels, uint32_t *h_labels, uint64_t *n_reps)
{
    const uint64_t n = c->n;
    const int descending = measure_descending(result_type) ? 1 : 0;
    const uint64_t band_floats = std::max<uint64_t>(c->threshold_band_bytes / sizeof(float), 1);
    HIPCHK(c, c->gr_assign.ensure(n * sizeof(uint32_t)));
    HIPCHK(c, c->gr_state.ensure(sizeof(uint64_t)));
    if (!d_labels) {
        HIPCHK(c, c->gr_labels.ensure(n * sizeof(uint32_t)));
        d_labels = (uint32_t *)c->gr_labels.ptr;
    }
    uint32_t *assign = (uint32_t *)c->gr_assign.ptr;
    uint64_t *d_reps = (uint64_t *)c->gr_state.ptr;
    HIPCHK(c, hipMemsetAsync(d_reps, 0, sizeof(uint64_t), c->stream));
    HIPCHK(c, launch_cc_init(c->stream, assign, n));  // assign[x] = x
    for (uint64_t b0 = 0; b0 + 1 < n;) {  // (the last row has no values)
        const uint64_t b1 = plan::greedy_band_end(n, b0, band_floats, c->greedy_band_rows);
        const uint64_t span = dsh_tri_span(n, b0, b1), longest = n - 1 - b0;
        const uint64_t nchunks64 = std::max<uint64_t>((longest + kThrChunk - 1) / kThrChunk, 1);
        if ((nchunks64 + 3) / 4 > 65535) return fail(c, DSH_EINVAL, "rows of %llu values are not supported", (unsigned long long)longest);
        ThrRows g;
        g.rect = 0;
        g.n = n;
        g.row0 = b0;
        g.ncols = 0;
        g.col0 = 0;
        g.rows = b1 - b0;
        g.nchunks = (uint32_t)nchunks64;
        HIPCHK(c, c->thr_vals.ensure(std::max<uint64_t>(span, 1) * sizeof(float)));
        if (span) {
            const int rc = run_pairs(c, PairJob::triangle(estim, result_type, k, b0, b1, dsh_tri_span(n, 0, b0), c->thr_vals.ptr));
            if (rc) return rc;
            const float *vals = (const float *)c->thr_vals.ptr;
            hipError_t e = launch_greedy_diag(c->stream, vals, g, t, descending, assign);
            if (e == hipSuccess) e = launch_greedy_band(c->stream, vals, g, t, descending, assign);
            if (e != hipSuccess) return fail(c, DSH_EIO, "k_greedy_diag/k_greedy_band: %s", hipGetErrorString(e));
        }
        b0 = b1;
    }
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
    if ((rc = greedy_bands(c, estim, result_type, k, t, d_labels, h_labels, n_reps))) return greedy_abort(c, rc);
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
