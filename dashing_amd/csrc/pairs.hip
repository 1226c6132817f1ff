// pairs.hip -- dsh_dist_pairs, dsh_dist_pairs_device, dsh_dist_pairs_csr: the values of an explicit list of pairs
// (DESIGN.md 4.8).  The direct form (kernels_pairs.hip): per pair the exact histogram of max(a, b), then the estimators of
// estimators.h -- the float32 the dense path writes for the same pair, bit for bit.  Nothing of the dense path's derived
// state (layout, planes, lists, keys, card) is read or written: the cardinalities this path needs are its own buffer.
// The list is worked off in chunks of "pairs_chunk" pairs, so scratch is 64 counters per pair of ONE chunk whatever the
// length of the list.
#include <algorithm>

#include "ctx.h"

using namespace dsh;

namespace dsh {

// (declared in ctx.h: group_stats.hip computes its pairs with the same machinery)
static size_t hist_bytes(const dsh_ctx *c, uint64_t cnt) { return cnt * 64 * (c->p <= kPairsMaxP16 ? 2 : 4); }

// the path's own cardinalities of all n sketches under `estim`: k_pairs_hist over the "pairs" (s, s), k_pairs_card.  A
// sketch with an out-of-range register is not reported here (it may never be named) -- it counts as empty.
int pairs_ensure_cards(dsh_ctx *c, int estim)
{
    if (c->pairs.card_estim == estim) return DSH_OK;
    c->pairs.card_estim = -1;
    HIPCHK(c, c->pairs.card.ensure(std::max<uint64_t>(c->n, 1) * sizeof(double)));
    const uint64_t chunk = c->pairs.chunk;
    HIPCHK(c, c->pairs.hist.ensure(hist_bytes(c, std::min<uint64_t>(chunk, std::max<uint64_t>(c->n, 1)))));
    for (uint64_t s0 = 0; s0 < c->n; s0 += chunk) {
        const uint64_t cnt = std::min<uint64_t>(chunk, c->n - s0);
        HIPCHK(c, launch_pairs_hist(c->stream, c->regs, c->n, c->p, nullptr, nullptr, s0, 0, cnt, c->pairs.hist.ptr, nullptr));
        HIPCHK(c, launch_pairs_card(c->stream, c->pairs.hist.ptr, s0, cnt, c->p, estim, (double *)c->pairs.card.ptr));
    }
    c->pairs.card_estim = estim;
    return DSH_OK;
}

int pairs_err_begin(dsh_ctx *c)
{
    HIPCHK(c, c->pairs.err.ensure(2 * sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->pairs.err.ptr, 0xFF, 2 * sizeof(unsigned long long), c->stream));
    return DSH_OK;
}

// one chunk: cnt pairs at d_lhs / d_rhs (device), values to out[t * out_stride + x]
int pairs_run_chunk(dsh_ctx *c, const PairsQuery &q, const uint32_t *d_lhs, const uint32_t *d_rhs, uint64_t xbase, uint64_t cnt,
                    float *d_out, uint64_t out_stride)
{
    const double ksinv = (double)(float)(1. / (double)q.k);  // the float 1/k of dist_loop (src/sketch_and_cmp.h:797)
    HIPCHK(c, c->pairs.hist.ensure(hist_bytes(c, cnt)));
    HIPCHK(c, launch_pairs_hist(c->stream, c->regs, c->n, c->p, d_lhs, d_rhs, 0, xbase, cnt, c->pairs.hist.ptr,
                                (unsigned long long *)c->pairs.err.ptr));
    HIPCHK(c, launch_pairs_finish(c->stream, c->pairs.hist.ptr, d_lhs, d_rhs, c->n, cnt, c->p, q.estim,
                                  (const double *)c->pairs.card.ptr, q.types, q.n_types, ksinv, d_out, out_stride));
    return DSH_OK;
}

// the one wait of a call: the error words, then the stream is idle
int pairs_err_end(dsh_ctx *c)
{
    unsigned long long e[2] = {~0ull, ~0ull};
    HIPCHK(c, hipMemcpyAsync(e, c->pairs.err.ptr, sizeof e, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (e[0] != ~0ull)
        return fail(c, DSH_EINVAL, "pair %llu names a slot outside [0, %llu)", e[0], (unsigned long long)c->n);
    if (e[1] != ~0ull)
        return fail(c, DSH_EINVAL, "sketch %llu holds a register value above %d (= 64 - p + 1): not an HLL of precision %d (corrupt or foreign .hll?)",
                    e[1], 64 - c->p + 1, c->p);
    return DSH_OK;
}

}  // namespace dsh

namespace {

int check_query(dsh_ctx *c, int estim, const int *result_types, uint32_t n_types, int k, PairsQuery &q)
{
    int rc = enter(c);
    if (rc) return rc;
    if (estim < 0 || estim > 2) return fail(c, DSH_EINVAL, "bad estimator %d", estim);
    if (n_types > 9) return fail(c, DSH_EINVAL, "%u result types: at most 9", n_types);
    if (n_types && !result_types) return DSH_EINVAL;
    if (k < 1) return fail(c, DSH_EINVAL, "bad k %d", k);
    q.estim = estim, q.k = k, q.n_types = n_types;
    for (uint32_t t = 0; t < 9; ++t) q.types.t[t] = 0;
    for (uint32_t t = 0; t < n_types; ++t) {
        if (result_types[t] < 0 || result_types[t] > 8) return fail(c, DSH_EINVAL, "unsupported result_type %d", result_types[t]);
        q.types.t[t] = result_types[t];
    }
    return DSH_OK;
}

// host forms: `fill(x0, cnt, lhs, rhs)` writes the pairs [x0, x0 + cnt) of the (already validated) list
template <class Fill>
int run_host(dsh_ctx *c, const PairsQuery &q, uint64_t n_pairs, const Fill &fill, float *out)
{
    if (!n_pairs || !q.n_types) return DSH_OK;
    int rc = pairs_ensure_cards(c, q.estim);
    if (rc || (rc = pairs_err_begin(c))) return rc;
    const uint64_t chunk = std::min<uint64_t>(c->pairs.chunk, n_pairs);
    HIPCHK(c, c->pairs.lhs.ensure(chunk * sizeof(uint32_t)));
    HIPCHK(c, c->pairs.rhs.ensure(chunk * sizeof(uint32_t)));
    HIPCHK(c, c->pairs.out.ensure(chunk * q.n_types * sizeof(float)));
    // the list travels through one page-locked slot (lhs then rhs of a chunk): it is rewritten once its upload has run
    // (the copy of a chunk's values into the caller's pageable `out` holds the host until the chunk is done anyway)
    HIPCHK(c, c->pairs.list.room(2 * chunk * sizeof(uint32_t)));
    uint32_t *hl = (uint32_t *)c->pairs.list.ptr(), *hr = hl + chunk;
    for (uint64_t x0 = 0; x0 < n_pairs && rc == DSH_OK; x0 += chunk) {
        const uint64_t cnt = std::min<uint64_t>(chunk, n_pairs - x0);
        if (c->pairs.list.wait() != hipSuccess) {  // (from the second chunk on: room() has waited for an earlier call's)
            rc = fail(c, DSH_EIO, "hipEventSynchronize failed");
            break;
        }
        fill(x0, cnt, hl, hr);
        if (hipMemcpyAsync(c->pairs.lhs.ptr, hl, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            hipMemcpyAsync(c->pairs.rhs.ptr, hr, cnt * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            c->pairs.list.sent(c->stream) != hipSuccess) {
            rc = fail(c, DSH_EIO, "upload of the pair list failed");
            break;
        }
        if ((rc = pairs_run_chunk(c, q, (const uint32_t *)c->pairs.lhs.ptr, (const uint32_t *)c->pairs.rhs.ptr, x0, cnt,
                            (float *)c->pairs.out.ptr, chunk)))
            break;
        for (uint32_t t = 0; t < q.n_types; ++t)
            if (hipMemcpyAsync(out + (uint64_t)t * n_pairs + x0, (const float *)c->pairs.out.ptr + (uint64_t)t * chunk,
                               cnt * sizeof(float), hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
                rc = fail(c, DSH_EIO, "copy of the values failed");
                break;
            }
    }
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        (void)hipGetLastError();
        return rc;
    }
    return pairs_err_end(c);
}

}  // namespace

extern "C" {

int dsh_dist_pairs(dsh_ctx *c, int estim, const int *result_types, uint32_t n_types, int k, const uint32_t *lhs,
                   const uint32_t *rhs, uint64_t n_pairs, float *out)
{
    PairsQuery q;
    int rc = check_query(c, estim, result_types, n_types, k, q);
    if (rc) return rc;
    if (n_pairs && (!lhs || !rhs)) return DSH_EINVAL;
    for (uint64_t x = 0; x < n_pairs; ++x)
        if (lhs[x] >= c->n || rhs[x] >= c->n)
            return fail(c, DSH_EINVAL, "pair %llu names a slot outside [0, %llu)", (unsigned long long)x, (unsigned long long)c->n);
    if (n_pairs && n_types && !out) return DSH_EINVAL;
    return run_host(c, q, n_pairs, [lhs, rhs](uint64_t x0, uint64_t cnt, uint32_t *l, uint32_t *r) {
        std::copy(lhs + x0, lhs + x0 + cnt, l);
        std::copy(rhs + x0, rhs + x0 + cnt, r);
    }, out);
}

int dsh_dist_pairs_device(dsh_ctx *c, int estim, const int *result_types, uint32_t n_types, int k, const void *d_lhs,
                          const void *d_rhs, uint64_t n_pairs, void *d_out)
{
    PairsQuery q;
    int rc = check_query(c, estim, result_types, n_types, k, q);
    if (rc) return rc;
    if (!n_pairs || !n_types) return DSH_OK;
    if (!d_lhs || !d_rhs || !d_out) return DSH_EINVAL;
    if ((rc = pairs_ensure_cards(c, q.estim)) || (rc = pairs_err_begin(c))) return rc;
    const uint64_t chunk = c->pairs.chunk;
    for (uint64_t x0 = 0; x0 < n_pairs; x0 += chunk) {
        const uint64_t cnt = std::min<uint64_t>(chunk, n_pairs - x0);
        if ((rc = pairs_run_chunk(c, q, (const uint32_t *)d_lhs + x0, (const uint32_t *)d_rhs + x0, x0, cnt, (float *)d_out + x0, n_pairs))) {
            (void)hipStreamSynchronize(c->stream);
            return rc;
        }
    }
    return pairs_err_end(c);
}

int dsh_dist_pairs_csr(dsh_ctx *c, int estim, const int *result_types, uint32_t n_types, int k, uint64_t row_begin,
                       uint64_t rows, const uint64_t *row_ptr, const uint32_t *col, float *out)
{
    PairsQuery q;
    int rc = check_query(c, estim, result_types, n_types, k, q);
    if (rc) return rc;
    if (!slots_ok(row_begin, rows, c->n)) return fail(c, DSH_EINVAL, "rows out of range");
    if (!rows) return DSH_OK;
    if (!row_ptr) return DSH_EINVAL;
    for (uint64_t r = 0; r < rows; ++r)
        if (row_ptr[r + 1] < row_ptr[r]) return fail(c, DSH_EINVAL, "row_ptr decreases at row %llu", (unsigned long long)r);
    const uint64_t h0 = row_ptr[0], n_hits = row_ptr[rows] - h0;  // (hit h of the call is col[h], h counted from row_ptr[0] on)
    if (n_hits && !col) return DSH_EINVAL;
    for (uint64_t h = 0; h < n_hits; ++h)
        if (col[h0 + h] >= c->n)
            return fail(c, DSH_EINVAL, "col[%llu] = %u outside [0, %llu)", (unsigned long long)(h0 + h), col[h0 + h], (unsigned long long)c->n);
    if (n_hits && n_types && !out) return DSH_EINVAL;
    uint64_t r = 0;  // row of the next hit to hand out (chunks are asked for in ascending order)
    return run_host(c, q, n_hits, [&](uint64_t x0, uint64_t cnt, uint32_t *l, uint32_t *rr) {
        for (uint64_t x = x0; x < x0 + cnt; ++x) {
            while (row_ptr[r + 1] - h0 <= x) ++r;
            l[x - x0] = col[h0 + x];
            rr[x - x0] = (uint32_t)(row_begin + r);
        }
    }, out);
}

}  // extern "C"
