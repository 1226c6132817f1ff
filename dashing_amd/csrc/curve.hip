// curve.hip -- dsh_union_curve, dsh_union_curve_device, dsh_curve_permutations: how the union of resident sketches grows
// along caller-given orders (kernels_curve.hip).  The calls read the resident rows and write the caller's
// buffers: nothing of the context's derived state is read or written.  Orders are worked off in batches whose deltas,
// start rows and counters stay within "curve_scratch_bytes" (curve_plan.h); a batch is: zero the deltas, with more than
// one segment per order the segments' unions (launch_union_groups) made start rows, the walk, the scan, and
// launch_pairs_card on the scanned counters.  No host wait between batches; one at the end, for the error word.
#include <algorithm>
#include <cstring>
#include <new>

#include "ctx.h"
#include "curve_plan.h"

using namespace dsh;

static_assert(curve::kScanChunk == kCurveScanChunk, "the planner sizes the chunk sums k_curve_scan* write");
static_assert(DSH_CURVE_BINS == 64, "a histogram is one lane per bin");

namespace {

struct CurveCall {
    int estim;
    uint64_t len, n_orders;
    curve::Plan plan;
};

// the checks both forms share, in the order of the contract; *empty: nothing to do
int check_call(dsh_ctx *c, int estim, uint64_t len, uint64_t n_orders, bool *empty)
{
    int rc = enter(c);
    if (rc) return rc;
    if (estim < 0 || estim > 2) return fail(c, DSH_EINVAL, "bad estimator %d", estim);
    *empty = !len || !n_orders;
    if (*empty) return DSH_OK;
    if (len >= curve::kMaxSteps || n_orders > ((uint64_t)1 << 48) / len)
        return fail(c, DSH_EINVAL, "%llu orders of %llu members: too many steps", (unsigned long long)n_orders, (unsigned long long)len);
    return DSH_OK;
}

int check_entries(dsh_ctx *c, const uint32_t *orders, uint64_t len, uint64_t n_orders)
{
    for (uint64_t o = 0; o < n_orders; ++o)
        for (uint64_t i = 0; i < len; ++i)
            if (orders[o * len + i] >= c->n)
                return fail(c, DSH_EINVAL, "order %llu, position %llu names slot %u outside [0, %llu)", (unsigned long long)o,
                            (unsigned long long)i, orders[o * len + i], (unsigned long long)c->n);
    return DSH_OK;
}

// plan, grow-only scratch, the error word and the segments' bounds of a full batch (a smaller last batch reads a prefix);
// `bounds` stays alive until the stream is idle
int begin(dsh_ctx *c, CurveCall &q, std::vector<uint64_t> &bounds)
{
    q.plan = curve::plan(q.n_orders, q.len, c->p, c->curve.scratch_bytes, c->curve.segment);
    const curve::Plan &pl = q.plan;
    const uint64_t B = pl.batch, wg_per_row = std::max<uint64_t>(((uint64_t)1 << c->p) >> 12, 1);
    if (pl.nseg >= curve::kMaxSteps || pl.nseg * wg_per_row >= curve::kMaxSteps)
        return fail(c, DSH_EINVAL, "an order of %llu members in segments of %llu: too many segments", (unsigned long long)q.len, (unsigned long long)pl.S);
    HIPCHK(c, c->curve.err.ensure(sizeof(unsigned long long)));
    HIPCHK(c, c->curve.delta.ensure(B * q.len * 256));
    HIPCHK(c, c->curve.cnt.ensure(B * q.len * 64 * (c->p <= kPairsMaxP16 ? 2 : 4)));
    if (pl.nchunk > 1) HIPCHK(c, c->curve.sums.ensure(B * pl.nchunk * 256));
    HIPCHK(c, hipMemsetAsync(c->curve.err.ptr, 0xFF, sizeof(unsigned long long), c->stream));
    if (pl.nseg > 1) {
        HIPCHK(c, c->curve.start.ensure((B * pl.nseg) << c->p));
        HIPCHK(c, c->curve.ptr.ensure((B * pl.nseg + 1) * sizeof(uint64_t)));
        bounds.resize(B * pl.nseg + 1);
        for (uint64_t o = 0; o < B; ++o)
            for (uint64_t s = 0; s < pl.nseg; ++s) bounds[o * pl.nseg + s] = o * q.len + pl.begin(s, q.len);
        bounds[B * pl.nseg] = B * q.len;
        HIPCHK(c, hipMemcpyAsync(c->curve.ptr.ptr, bounds.data(), bounds.size() * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
    }
    return DSH_OK;
}

// one batch: the orders [o0, o0 + cnt) at d_ord (device, the batch's first entry); cardinalities to d_card[0 .. cnt * len),
// histograms to d_hist (or nullptr)
int run_batch(dsh_ctx *c, const CurveCall &q, const uint32_t *d_ord, uint64_t cnt, double *d_card, uint32_t *d_hist)
{
    const curve::Plan &pl = q.plan;
    const int p = c->p;
    HIPCHK(c, hipMemsetAsync(c->curve.delta.ptr, 0, cnt * q.len * 256, c->stream));
    uint8_t *start = nullptr;
    if (pl.nseg > 1) {
        start = (uint8_t *)c->curve.start.ptr;
        HIPCHK(c, launch_union_groups(c->stream, c->regs, p, (const uint64_t *)c->curve.ptr.ptr, d_ord, nullptr, cnt * pl.nseg, start, nullptr));
        HIPCHK(c, launch_curve_starts(c->stream, start, p, pl.nseg, cnt));
    }
    HIPCHK(c, launch_curve_walk(c->stream, c->regs, c->n, p, d_ord, q.len, pl.S, pl.nseg, cnt, start, (int *)c->curve.delta.ptr,
                                (unsigned long long *)c->curve.err.ptr));
    HIPCHK(c, launch_curve_scan(c->stream, (const int *)c->curve.delta.ptr, (int *)c->curve.sums.ptr, q.len, cnt, p, c->curve.cnt.ptr, d_hist));
    HIPCHK(c, launch_pairs_card(c->stream, c->curve.cnt.ptr, 0, cnt * q.len, p, q.estim, d_card));
    return DSH_OK;
}

// the one wait of a call: the error word, then the stream is idle
int finish(dsh_ctx *c)
{
    unsigned long long e = ~0ull;
    HIPCHK(c, hipMemcpyAsync(&e, c->curve.err.ptr, sizeof e, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (e != ~0ull)
        return fail(c, DSH_EINVAL, "sketch %llu holds a register value above %d (= 64 - p + 1): not an HLL of precision %d (corrupt or foreign .hll?)",
                    e, 64 - c->p + 1, c->p);
    return DSH_OK;
}

inline uint64_t splitmix64(uint64_t &x)
{
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

}  // namespace

extern "C" {

int dsh_union_curve_device(dsh_ctx *c, int estim, const void *d_orders, uint64_t len, uint64_t n_orders, void *d_card, void *d_hist)
{
    bool empty = false;
    int rc = check_call(c, estim, len, n_orders, &empty);
    if (rc || empty) return rc;
    if (!d_orders || !d_card) return DSH_EINVAL;
    // the entries are judged on the host before anything is launched, as the host form's are: 4 bytes per step come back,
    // against the 2^p the walk reads for it
    std::vector<uint32_t> h;
    try {
        h.resize(n_orders * len);
    } catch (const std::bad_alloc &) {
        return fail(c, DSH_ENOMEM, "no host memory for %llu order entries", (unsigned long long)(n_orders * len));
    }
    HIPCHK(c, hipMemcpyAsync(h.data(), d_orders, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if ((rc = check_entries(c, h.data(), len, n_orders))) return rc;
    CurveCall q{estim, len, n_orders, {}};
    std::vector<uint64_t> bounds;
    if ((rc = begin(c, q, bounds))) return drain(c, rc);
    for (uint64_t o0 = 0; o0 < n_orders; o0 += q.plan.batch) {
        const uint64_t cnt = std::min(q.plan.batch, n_orders - o0);
        if ((rc = run_batch(c, q, (const uint32_t *)d_orders + o0 * len, cnt, (double *)d_card + o0 * len,
                            d_hist ? (uint32_t *)d_hist + o0 * len * 64 : nullptr)))
            return drain(c, rc);
    }
    return finish(c);
}

int dsh_union_curve(dsh_ctx *c, int estim, const uint32_t *orders, uint64_t len, uint64_t n_orders, double *card_out, uint32_t *hist_out)
{
    bool empty = false;
    int rc = check_call(c, estim, len, n_orders, &empty);
    if (rc || empty) return rc;
    if (!orders || !card_out) return DSH_EINVAL;
    if ((rc = check_entries(c, orders, len, n_orders))) return rc;
    CurveCall q{estim, len, n_orders, {}};
    std::vector<uint64_t> bounds;
    const uint64_t steps = n_orders * len;
    // the orders (4 bytes per step) and the cardinalities (8) are held whole, the histograms (256) per batch
    HIPCHK(c, c->curve.ord.ensure(steps * sizeof(uint32_t)));
    HIPCHK(c, c->curve.card.ensure(steps * sizeof(double)));
    HIPCHK(c, hipMemcpyAsync(c->curve.ord.ptr, orders, steps * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = begin(c, q, bounds))) return drain(c, rc);
    const uint64_t B = q.plan.batch;
    const bool one = B >= n_orders;
    // an error found on the device (a register out of range) is only known at the end: the histograms of a call of several
    // batches wait in host memory of the library's until then, so that a failed call leaves hist_out as it was
    std::vector<uint32_t> held;
    if (hist_out) {
        HIPCHK(c, c->curve.hist.ensure(std::min(B, n_orders) * len * 256));
        if (!one) {
            try {
                held.resize(steps * 64);
            } catch (const std::bad_alloc &) {
                return drain(c, fail(c, DSH_ENOMEM, "no host memory for %llu histograms", (unsigned long long)steps));
            }
        }
    }
    for (uint64_t o0 = 0; o0 < n_orders; o0 += B) {
        const uint64_t cnt = std::min(B, n_orders - o0);
        if ((rc = run_batch(c, q, (const uint32_t *)c->curve.ord.ptr + o0 * len, cnt, (double *)c->curve.card.ptr + o0 * len,
                            hist_out ? (uint32_t *)c->curve.hist.ptr : nullptr)))
            return drain(c, rc);
        if (hist_out && !one &&
            hipMemcpyAsync(held.data() + o0 * len * 64, c->curve.hist.ptr, cnt * len * 256, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            return drain(c, fail(c, DSH_EIO, "copy of the histograms of orders %llu.. failed", (unsigned long long)o0));
    }
    if ((rc = finish(c))) return rc;
    HIPCHK(c, hipMemcpyAsync(card_out, c->curve.card.ptr, steps * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (hist_out && one) HIPCHK(c, hipMemcpyAsync(hist_out, c->curve.hist.ptr, steps * 256, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (hist_out && !one) std::memcpy(hist_out, held.data(), steps * 256);
    return DSH_OK;
}

int dsh_curve_permutations(uint64_t n, uint64_t n_perm, uint64_t seed, uint32_t *out)
{
    if (n >= ((uint64_t)1 << 32)) return DSH_EINVAL;
    if (!n || !n_perm) return DSH_OK;
    if (!out) return DSH_EINVAL;
    for (uint64_t r = 0; r < n_perm; ++r) {
        uint32_t *row = out + r * n;
        for (uint64_t i = 0; i < n; ++i) row[i] = (uint32_t)i;
        uint64_t x = seed + r;
        for (uint64_t i = n - 1; i >= 1; --i) std::swap(row[i], row[splitmix64(x) % (i + 1)]);
    }
    return DSH_OK;
}

}  // extern "C"
