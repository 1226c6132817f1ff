// abi.hip -- the C-ABI of libdashing_hip.so (include/dashing_hip.h) over the gfx950 kernels: context, resident sketch
// matrix, cardinalities, the compare entry points, per-call completion tickets, shards of the sorted triangle, options.
// Argument checks and call sequencing live here; the work is in engine.hip (prepare / run_pairs), knn.hip,
// comm.hip and exchange.hip; the sketch entry points are sketch.hip's; the pure entry points (dsh_tri_*, dsh_partition_rows,
// dsh_balance_rows, dsh_range_parts) and the shard bounds are in plan.cpp.  No CPU fallback lives here: without a HIP
// device dsh_create fails with DSH_ENODEV.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "ctx.h"

using namespace dsh;

extern "C" {

const char *dsh_backend_name(void) { return "hip:gfx950"; }

int dsh_abi_version(void) { return DSH_ABI_VERSION; }

int dsh_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The explicit part of a teardown, for dsh_destroy and the failure path of dsh_create: the device is made current and
// every stream waited for (nothing of ours is then in flight), the spin kernel let go, the communicator destroyed while
// its library is loaded.  `delete` then frees the buffers, staging blocks and events, and the streams last (ctx.h: the
// order of the members).
static void release_ctx(dsh_ctx *c)
{
    (void)hipSetDevice(c->device);
    for (const Stream *s : {&c->stream, &c->copy_stream, &c->aux_stream, &c->place_stream})
        if (*s) (void)hipStreamSynchronize(*s);
    if (c->xch.spin_running && c->xch.spin_flag.ptr) *(volatile uint32_t *)c->xch.spin_flag.ptr = 1;
    if (c->spin_stream) (void)hipStreamSynchronize(c->spin_stream);
    c->xch.spin_running = false;
    (void)comm_release(c);
}

int dsh_create(int device, dsh_ctx **out)
{
    if (!out) return DSH_EINVAL;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return DSH_ENODEV;
    if (device < 0 || device >= n) return DSH_EINVAL;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return DSH_ENODEV;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return DSH_ENODEV;  // gfx950-only code object
    dsh_ctx *c = new (std::nothrow) dsh_ctx;
    if (!c) return DSH_ENOMEM;
    c->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        c->stream.create() != hipSuccess || c->copy_stream.create_copy() != hipSuccess ||
        c->aux_stream.create() != hipSuccess || c->place_stream.create_copy() != hipSuccess ||
        c->ev_aux_fork.ensure() != hipSuccess || c->ev_aux_join.ensure() != hipSuccess) {
        release_ctx(c);
        delete c;
        return DSH_EIO;
    }
    *out = c;
    return DSH_OK;
}

void dsh_destroy(dsh_ctx *c)
{
    if (!c) return;
    release_ctx(c);
    delete c;
}

int dsh_preload(int device, unsigned what)
{
    if (hipSetDevice(device) != hipSuccess) {
        (void)hipGetLastError();  // (the runtime keeps the last error per thread: a later launch's check must not find this one)
        return DSH_ENODEV;
    }
    hipError_t e = hipSuccess;
    if ((what & DSH_PRELOAD_SKETCH) && e == hipSuccess) e = preload_sketch_kernels();
    if ((what & DSH_PRELOAD_SKETCH) && e == hipSuccess) e = preload_fastx_kernels();
    if ((what & DSH_PRELOAD_COMPARE) && e == hipSuccess) e = preload_compare_kernels();
    if ((what & DSH_PRELOAD_COMPARE) && e == hipSuccess) e = preload_hist_kernels();
    if ((what & DSH_PRELOAD_COMPARE) && e == hipSuccess) e = preload_sparseplane_kernels();
    if ((what & DSH_PRELOAD_COMPARE) && e == hipSuccess) e = preload_knn_kernels();
    if ((what & DSH_PRELOAD_COMPARE) && e == hipSuccess) e = preload_exchange_kernels();
    if (e != hipSuccess) (void)hipGetLastError();
    return e == hipSuccess ? DSH_OK : DSH_EIO;
}

const char *dsh_last_error(const dsh_ctx *c) { return c ? c->err.c_str() : "null ctx"; }

int dsh_synchronize(dsh_ctx *c)
{
    if (!c) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    HIPCHK(c, hipStreamSynchronize(c->place_stream));
    return DSH_OK;
}

void *dsh_stream(dsh_ctx *c) { return c ? (void *)c->stream : nullptr; }

int dsh_sketches_alloc(dsh_ctx *c, uint64_t n, int p)
{
    if (!c) return DSH_EINVAL;
    if (p < 4 || p > kMaxP) return fail(c, DSH_EINVAL, "p=%d outside [4,%d]", p, kMaxP);
    int rc = bind(c);
    if (rc) return rc;
    const size_t bytes = std::max<size_t>((size_t)n << p, 256);
    HIPCHK(c, c->regs_own.ensure(bytes));
    HIPCHK(c, hipMemsetAsync(c->regs_own.ptr, 0, bytes, c->stream));
    c->regs = (const uint8_t *)c->regs_own.ptr;
    c->n = n;
    c->p = p;
    c->have_sketches = true;
    invalidate(c);
    return DSH_OK;
}

int dsh_attach_device_sketches(dsh_ctx *c, const void *d_regs, uint64_t n, int p)
{
    if (!c || (!d_regs && n)) return DSH_EINVAL;
    if (p < 4 || p > kMaxP) return fail(c, DSH_EINVAL, "p=%d outside [4,%d]", p, kMaxP);
    if (((uintptr_t)d_regs & 15) != 0) return fail(c, DSH_EINVAL, "device sketches must be 16-byte aligned");
    c->regs = (const uint8_t *)d_regs;
    c->n = n;
    c->p = p;
    c->have_sketches = true;
    invalidate(c);
    return DSH_OK;
}

int dsh_upload_sketches(dsh_ctx *c, const uint8_t *regs, uint64_t first, uint64_t n)
{
    if (!c || (!regs && n)) return DSH_EINVAL;
    if (!c->have_sketches || c->regs != (const uint8_t *)c->regs_own.ptr)
        return fail(c, DSH_ESTATE, "dsh_sketches_alloc first");
    if (!slots_ok(first, n, c->n)) return fail(c, DSH_EINVAL, "slots [%llu,+%llu) out of range", (unsigned long long)first, (unsigned long long)n);
    int rc = bind(c);
    if (rc) return rc;
    if (n) {
        HIPCHK(c, hipMemcpyAsync((uint8_t *)c->regs_own.ptr + (first << c->p), regs, (size_t)n << c->p,
                                 hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    invalidate(c);
    return DSH_OK;
}

int dsh_download_sketches(dsh_ctx *c, uint64_t first, uint64_t n, uint8_t *out)
{
    if (!c || (!out && n)) return DSH_EINVAL;
    if (!c->have_sketches) return fail(c, DSH_ESTATE, "no sketches");
    if (!slots_ok(first, n, c->n)) return fail(c, DSH_EINVAL, "slots out of range");
    int rc = bind(c);
    if (rc) return rc;
    if (n) {
        HIPCHK(c, hipMemcpyAsync(out, c->regs + (first << c->p), (size_t)n << c->p,
                                 hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return DSH_OK;
}

int dsh_copy_sketches_device(dsh_ctx *c, uint64_t first, uint64_t n, void *d_out)
{
    if (!c || (!d_out && n)) return DSH_EINVAL;
    if (!c->have_sketches) return fail(c, DSH_ESTATE, "no sketches");
    if (!slots_ok(first, n, c->n)) return fail(c, DSH_EINVAL, "slots out of range");
    int rc = bind(c);
    if (rc) return rc;
    if (n) {
        HIPCHK(c, hipMemcpyAsync(d_out, c->regs + (first << c->p), (size_t)n << c->p,
                                 hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return DSH_OK;
}

int dsh_clear_sketches(dsh_ctx *c, uint64_t first, uint64_t n)
{
    if (!c) return DSH_EINVAL;
    if (!c->have_sketches || c->regs != (const uint8_t *)c->regs_own.ptr)
        return fail(c, DSH_ESTATE, "dsh_sketches_alloc first");
    if (!slots_ok(first, n, c->n)) return fail(c, DSH_EINVAL, "slots out of range");
    int rc = bind(c);
    if (rc) return rc;
    if (n) HIPCHK(c, hipMemsetAsync((uint8_t *)c->regs_own.ptr + (first << c->p), 0, (size_t)n << c->p, c->stream));
    invalidate(c);
    return DSH_OK;
}

int dsh_cardinalities(dsh_ctx *c, int estim, double *out)
{
    if (!c || !out) return DSH_EINVAL;
    int rc = enter(c);
    if (rc) return rc;
    if (estim < 0 || estim > 2) return fail(c, DSH_EINVAL, "bad estimator %d", estim);
    if (c->card_estim != estim || c->card_from != 0) {
        // same per-sketch pass as prepare() (thresholds/exception lists come out identical)
        rc = prepare(c, estim, -1, /*card_only=*/true);
        if (rc) return rc;
    }
    if (c->n) {
        HIPCHK(c, hipMemcpyAsync(out, c->card.ptr, c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
}

int dsh_dist_rows_device_async(dsh_ctx *c, int estim, int result_type, int k, uint64_t rb, uint64_t re, void *d_out)
{
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    if (re > c->n) re = c->n;
    if (rb >= re || c->n < 2) return DSH_OK;
    if (!d_out) return DSH_EINVAL;
    return run_pairs(c, PairJob::triangle(estim, result_type, k, rb, re, dsh_tri_span(c->n, 0, rb), d_out));
}

int dsh_dist_rows_parts_device_async(dsh_ctx *c, int estim, int result_type, int k, uint64_t rb, uint64_t re, void *d_out,
                                     uint32_t nparts)
{
    if (!c || nparts == 0) return DSH_EINVAL;
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    c->parts_done = 0;
    if (re > c->n) re = c->n;
    if (rb >= re || c->n < 2) return DSH_OK;  // (no rows: no parts, no events -- dsh_collect_parts_async knows)
    if (!d_out) return DSH_EINVAL;
    PairJob j = PairJob::triangle(estim, result_type, k, rb, re, dsh_tri_span(c->n, 0, rb), d_out);
    j.nparts = nparts;
    return run_pairs(c, j);
}

int dsh_dist_rows_device(dsh_ctx *c, int estim, int result_type, int k, uint64_t rb, uint64_t re, void *d_out)
{
    int rc = dsh_dist_rows_device_async(c, estim, result_type, k, rb, re, d_out);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
}

int dsh_dist_rows_async(dsh_ctx *c, int estim, int result_type, int k, uint64_t rb, uint64_t re, float *out)
{
    int rc = enter(c);
    if (rc) return rc;
    if (re > c->n) re = c->n;
    const uint64_t span = dsh_tri_span(c->n, rb, re);
    if (span == 0) return DSH_OK;
    if (!out) return DSH_EINVAL;
    // Two device buffers taken in turn: this call's kernels (ctx stream) wait only for the copy that last drained
    // THEIR buffer, so they run while the previous call's result is still on its way to the host (copy stream) --
    // the reference overlaps the comparison of one batch of rows with the emission of the previous one the same way
    // (src/sketch_and_cmp.h:804-816, distmat/distmat.h:475-479,504-508).
    const unsigned b = c->out_turn++ & 1u;
    for (int t = 0; t < 2; ++t) {
        HIPCHK(c, c->ev_filled[t].ensure());
        HIPCHK(c, c->ev_drained[t].ensure());
    }
    if (c->outbuf2[b].cap < span * sizeof(float)) {  // growing frees the old buffer: let its last copy finish first
        if (c->drained_pending[b]) HIPCHK(c, hipEventSynchronize(c->ev_drained[b]));
        c->drained_pending[b] = false;
        HIPCHK(c, c->outbuf2[b].ensure(span * sizeof(float)));
    }
    if (c->drained_pending[b]) HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_drained[b], 0));
    rc = dsh_dist_rows_device_async(c, estim, result_type, k, rb, re, c->outbuf2[b].ptr);
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev_filled[b], c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_filled[b], 0));
    HIPCHK(c, hipMemcpyAsync(out, c->outbuf2[b].ptr, span * sizeof(float), hipMemcpyDeviceToHost, c->copy_stream));
    HIPCHK(c, hipEventRecord(c->ev_drained[b], c->copy_stream));
    c->drained_pending[b] = true;
    return DSH_OK;
}

int dsh_dist_rows(dsh_ctx *c, int estim, int result_type, int k, uint64_t rb, uint64_t re, float *out)
{
    int rc = dsh_dist_rows_async(c, estim, result_type, k, rb, re, out);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipStreamSynchronize(c->copy_stream));
    return DSH_OK;
}

int dsh_wait(dsh_ctx *c) { return dsh_synchronize(c); }

// A ticket marks "everything enqueued on this ctx so far" (kernels on the ctx stream and the copies of
// dsh_dist_rows_async / transfers of dsh_collect_parts_async on the copy stream); waiting for it does not wait for work
// enqueued afterwards.  It is TWO independent events, one per stream, and orders nothing between the streams: a ticket
// taken between the compute call and dsh_collect_parts_async does not hold the per-part transfers behind the kernels.
static constexpr size_t kTicketRing = 64;

int dsh_event_record(dsh_ctx *c, uint64_t *ticket)
{
    if (!c || !ticket) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    if (c->tickets.size() < 2 * kTicketRing) {
        HIPCHK(c, add_event(c->tickets));
        HIPCHK(c, add_event(c->tickets));
    }
    const uint64_t t = c->ticket_next;
    hipEvent_t es = c->tickets[2 * (t % kTicketRing)], ec = c->tickets[2 * (t % kTicketRing) + 1];
    if (t >= kTicketRing) {  // the ticket that used this slot 64 records ago
        HIPCHK(c, hipEventSynchronize(es));
        HIPCHK(c, hipEventSynchronize(ec));
    }
    HIPCHK(c, hipEventRecord(es, c->stream));
    HIPCHK(c, hipEventRecord(ec, c->copy_stream));
    c->ticket_next = t + 1;
    *ticket = t;
    return DSH_OK;
}

static int ticket_events(dsh_ctx *c, uint64_t ticket, hipEvent_t e[2])
{
    if (ticket >= c->ticket_next) return fail(c, DSH_EINVAL, "ticket %llu was never recorded", (unsigned long long)ticket);
    e[0] = e[1] = nullptr;
    if (c->ticket_next - ticket <= kTicketRing) {  // (older than the ring: waited for when its slot was reused)
        e[0] = c->tickets[2 * (ticket % kTicketRing)];
        e[1] = c->tickets[2 * (ticket % kTicketRing) + 1];
    }
    return DSH_OK;
}

int dsh_event_wait(dsh_ctx *c, uint64_t ticket)
{
    if (!c) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    hipEvent_t e[2];
    if ((rc = ticket_events(c, ticket, e))) return rc;
    for (hipEvent_t x : e)
        if (x) HIPCHK(c, hipEventSynchronize(x));
    return DSH_OK;
}

int dsh_event_query(dsh_ctx *c, uint64_t ticket, int *done)
{
    if (!c || !done) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    hipEvent_t e[2];
    if ((rc = ticket_events(c, ticket, e))) return rc;
    *done = 1;
    for (hipEvent_t x : e) {
        if (!x) continue;
        const hipError_t q = hipEventQuery(x);
        if (q == hipErrorNotReady) *done = 0;
        else if (q != hipSuccess) return fail(c, DSH_EIO, "hipEventQuery: %s", hipGetErrorString(q));
    }
    return DSH_OK;
}

int dsh_wait_event(dsh_ctx *c, void *hip_event)
{
    if (!c || !hip_event) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamWaitEvent(c->stream, (hipEvent_t)hip_event, 0));
    return DSH_OK;
}

int dsh_dist_rect(dsh_ctx *c, int estim, int result_type, int k, uint64_t qb, uint64_t qe, uint64_t rb, uint64_t re, float *out)
{
    int rc = enter(c);
    if (rc) return rc;
    if (qe > c->n || re > c->n) return fail(c, DSH_EINVAL, "slots out of range");
    reset_prof(c);
    if (qb >= qe || rb >= re) return DSH_OK;
    if (!out) return DSH_EINVAL;
    const uint64_t cnt = (qe - qb) * (re - rb);
    HIPCHK(c, c->outbuf.ensure(cnt * sizeof(float)));
    rc = run_pairs(c, PairJob::rectangle(estim, result_type, k, qb, qe, rb, re, c->outbuf.ptr));
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(out, c->outbuf.ptr, cnt * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
}

// where shard r of the bounds tb (plan::shard_bounds) begins in the sorted triangle (r = nshards: where the last ends)
static uint64_t shard_off(const dsh_ctx *c, const std::vector<uint32_t> &tb, uint32_t r)
{
    return dsh_tri_span(c->n, 0, plan::shard_row(tb, r, c->n));
}

int dsh_shard_plan(dsh_ctx *c, int estim, uint32_t nshards, uint64_t *span_off)
{
    if (!c || !span_off || nshards == 0) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    if ((rc = prepare(c, estim, 1))) return rc;
    std::vector<uint32_t> tb;
    plan::shard_bounds(c->lay, nshards, tb);
    for (uint32_t r = 0; r <= nshards; ++r) span_off[r] = shard_off(c, tb, r);
    return DSH_OK;
}

int dsh_dist_shard_device(dsh_ctx *c, int estim, int result_type, int k, uint32_t shard,
                          uint32_t nshards, void *d_span)
{
    if (!c || nshards == 0 || shard >= nshards) return DSH_EINVAL;
    int rc = enter(c);
    if (rc) return rc;
    reset_prof(c);
    if ((rc = prepare(c, estim, 1))) return rc;
    if (c->n < 2) return DSH_OK;
    std::vector<uint32_t> tb;
    plan::shard_bounds(c->lay, nshards, tb);
    const uint64_t sb = plan::shard_row(tb, shard, c->n), se = plan::shard_row(tb, shard + 1, c->n);
    PairJob j = PairJob::triangle(estim, result_type, k, sb, se, dsh_tri_span(c->n, 0, sb), d_span);
    j.sorted_rows = 1;
    if (j.row_begin >= j.row_end) return DSH_OK;
    if (!d_span) return DSH_EINVAL;
    if ((rc = run_pairs(c, j))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
}

int dsh_unpermute_device(dsh_ctx *c, const void *d_sorted_tri, void *d_out_tri)
{
    if (!c) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    if (!whole_sorted(c)) return fail(c, DSH_ESTATE, "no sorted plan (call dsh_shard_plan / dsh_dist_shard_device first)");
    if (c->n < 2) return DSH_OK;
    if (!d_sorted_tri || !d_out_tri) return DSH_EINVAL;
    HIPCHK(c, launch_unpermute(c->stream, (const float *)d_sorted_tri, (const uint32_t *)c->perm.ptr + c->n, c->n, (float *)d_out_tri));
    return DSH_OK;
}

// What the two staged un-permutes start with: the state check, and the shard bounds computed once.  tb stays empty where
// there is nothing to do (fewer than two sketches).
static int unpermute_bounds(dsh_ctx *c, uint32_t nshards, std::vector<uint32_t> &tb)
{
    int rc = bind(c);
    if (rc) return rc;
    if (!whole_sorted(c)) return fail(c, DSH_ESTATE, "no sorted plan (call dsh_shard_plan / dsh_dist_shard_device first)");
    if (c->n >= 2) plan::shard_bounds(c->lay, nshards, tb);
    return DSH_OK;
}

// shard r of the bounds tb lies at block_off[r] of d_stage
static int unpermute_blocks(dsh_ctx *c, const void *d_stage, const uint64_t *block_off, uint32_t nshards, void *d_out_tri,
                            const std::vector<uint32_t> &tb)
{
    if (!d_stage || !d_out_tri) return DSH_EINVAL;
    const uint32_t NT = c->lay.Npad / kTile;
    std::vector<int64_t> delta(NT, 0);
    for (uint32_t r = 0; r < nshards; ++r)
        for (uint32_t t = tb[r]; t < tb[r + 1]; ++t) delta[t] = (int64_t)block_off[r] - (int64_t)shard_off(c, tb, r);
    HIPCHK(c, c->sketch.workbuf.ensure(NT * sizeof(int64_t)));
    HIPCHK(c, hipMemcpyAsync(c->sketch.workbuf.ptr, delta.data(), NT * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_unpermute_staged(c->stream, (const float *)d_stage, (const uint32_t *)c->perm.ptr + c->n,
                                      (const int64_t *)c->sketch.workbuf.ptr, c->n, (float *)d_out_tri));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // `delta` (pageable source) must outlive the copy
    return DSH_OK;
}

int dsh_unpermute_blocks_device(dsh_ctx *c, const void *d_stage, const uint64_t *block_off, uint32_t nshards, void *d_out_tri)
{
    if (!c || nshards == 0 || !block_off) return DSH_EINVAL;
    std::vector<uint32_t> tb;
    const int rc = unpermute_bounds(c, nshards, tb);
    if (rc || tb.empty()) return rc;
    return unpermute_blocks(c, d_stage, block_off, nshards, d_out_tri, tb);
}

int dsh_unpermute_staged_device(dsh_ctx *c, const void *d_stage, uint64_t stride, uint32_t nshards, void *d_out_tri)
{
    if (!c || nshards == 0) return DSH_EINVAL;
    std::vector<uint32_t> tb;
    const int rc = unpermute_bounds(c, nshards, tb);
    if (rc || tb.empty()) return rc;
    std::vector<uint64_t> off(nshards);
    for (uint32_t r = 0; r < nshards; ++r) {  // the spans must fit their blocks
        if (shard_off(c, tb, r + 1) - shard_off(c, tb, r) > stride)
            return fail(c, DSH_EINVAL, "stride %llu smaller than the span of shard %u", (unsigned long long)stride, r);
        off[r] = (uint64_t)r * stride;
    }
    return unpermute_blocks(c, d_stage, off.data(), nshards, d_out_tri, tb);
}

void *dsh_alloc_host(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}

void dsh_free_host(void *p)
{
    if (p) (void)hipHostFree(p);
}

int dsh_set_profiling(dsh_ctx *c, int enable)
{
    if (!c) return DSH_EINVAL;
    c->profiling = enable != 0;
    if (!c->profiling) c->finalize_stop = c->finalize_timing = 0;  // the stop points and stamps exist for profiling runs only
    return DSH_OK;
}

int dsh_last_kernel_ms(dsh_ctx *c, double *pair_ms, double *fin_ms, double *prep_ms, uint32_t *launches)
{
    if (!c) return DSH_EINVAL;
    if (pair_ms) *pair_ms = c->pair_ms;
    if (fin_ms) *fin_ms = c->fin_ms;
    if (prep_ms) *prep_ms = c->prep_ms;
    if (launches) *launches = c->pair_launches;
    return DSH_OK;
}

int dsh_last_part_info(dsh_ctx *c, double *ready_ms, uint64_t *floats, uint32_t cap, uint32_t *nparts_out)
{
    if (!c || !nparts_out) return DSH_EINVAL;
    const uint32_t k = (uint32_t)c->part_ready_ms.size();
    *nparts_out = k;
    if (k > cap && (ready_ms || floats)) return DSH_EINVAL;
    for (uint32_t q = 0; q < k; ++q) {
        if (ready_ms) ready_ms[q] = c->part_ready_ms[q];
        if (floats) floats[q] = c->part_floats[q];
    }
    return DSH_OK;
}

int dsh_finalize_phase_cycles(dsh_ctx *c, uint64_t *out16)
{
    if (!c || !out16) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    if (!c->phase_cyc.ptr) return fail(c, DSH_ESTATE, "no call with the option finalize_timing yet");
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(out16, c->phase_cyc.ptr, 16 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return DSH_OK;
}

int dsh_get_info(dsh_ctx *c, const char *name, int64_t *out)
{
    if (!c || !name || !out) return DSH_EINVAL;
    if (!std::strcmp(name, "planes")) *out = c->lay.P;
    else if (!std::strcmp(name, "vlo")) *out = c->lay.vlo;
    else if (!std::strcmp(name, "vhi")) *out = c->lay.vhi;
    else if (!std::strcmp(name, "threshold")) *out = c->lay.pbase + (int64_t)c->lay.P;
    else if (!std::strcmp(name, "pbase")) *out = c->lay.pbase;
    else if (!std::strcmp(name, "host_layout_us")) *out = (int64_t)c->host_layout_us;
    else if (!std::strcmp(name, "host_lists_us")) *out = (int64_t)c->host_lists_us;
    else if (!std::strcmp(name, "host_keys_wait_us")) *out = (int64_t)c->host_keys_wait_us;
    else if (!std::strcmp(name, "host_sparse_us")) *out = (int64_t)c->host_sparse_us;  // the sparse items' emission (plan.h), behind the first tile kernel
    else if (!std::strcmp(name, "emax")) *out = c->emax;
    else if (!std::strcmp(name, "elow")) *out = c->elow;
    else if (!std::strcmp(name, "kc")) *out = c->kc;
    else if (!std::strcmp(name, "pair_groups")) *out = c->pair_groups;
    else if (!std::strcmp(name, "pair_round")) *out = c->pp.band_round.empty() ? 0 : c->pp.band_round[0];  // the round the last call's first band ran in
    else if (!std::strcmp(name, "tile")) *out = kTile;
    else if (!std::strcmp(name, "parts_done")) *out = c->parts_done;
    else if (!std::strcmp(name, "parts_signalled")) *out = c->parts_signalled ? 1 : 0;
    else if (!std::strcmp(name, "sketch_kernel_us")) *out = (int64_t)(c->sketch_ms * 1000.0);
    else if (!std::strcmp(name, "fastx_decode_us")) *out = (int64_t)(c->fastx_ms * 1000.0);
    else if (!std::strcmp(name, "xch_recv_gated")) *out = c->xch.recv_gated ? 1 : 0;
    else if (!std::strcmp(name, "stats_route")) *out = c->gs.route_last;
    else if (!std::strcmp(name, "linkage_route")) *out = c->lk.route_last;
    else if (!std::strcmp(name, "mst_rounds")) *out = c->mst.rounds_last;
    else if (!std::strcmp(name, "mst_band_us")) *out = (int64_t)(c->mst.band_ms * 1000.0);
    else if (!std::strcmp(name, "place_kernel_us")) *out = (int64_t)(c->xch.place_ms * 1000.0);
    else if (!std::strcmp(name, "whatif_mfma")) {
#ifdef DSH_WHATIF_MFMA
        *out = 1;
#else
        *out = 0;
#endif
    }
    else if (!std::strcmp(name, "npad")) *out = c->lay.Npad;
    else if (!std::strcmp(name, "kpad")) *out = c->Kpad;
    else if (!std::strcmp(name, "cum_bytes")) *out = c->cum_bytes;
    else if (!std::strcmp(name, "sorted")) *out = c->lay.sorted;
    else if (!std::strcmp(name, "ncols")) *out = (int64_t)c->lay.ncols;
    else if (!std::strcmp(name, "lockstep")) *out = c->planes_valid && use_lockstep(c) ? 1 : 0;
    else if (!std::strcmp(name, "tiles")) *out = (int64_t)c->pp.T.size();
    else if (!std::strcmp(name, "bands")) *out = (int64_t)c->last_bands;
    else if (!std::strcmp(name, "items")) *out = (int64_t)c->pp.items.size();  // work items of the tile kernel (rounds of 256 x pair_groups)
    else if (!std::strcmp(name, "frag_items")) {  // ... of which overflow fragments (plan.h)
        uint64_t f = 0;
        for (uint32_t x : c->pp.band_frags) f += x;
        *out = (int64_t)f;
    }
    else if (!std::strcmp(name, "sparse_items")) *out = (int64_t)c->pp.sp_items.size();  // (tile, plane) items counted from position lists (plan.h)
    else if (!std::strcmp(name, "sparse_plane_us")) *out = (int64_t)(c->sparse_ms * 1000.0);  // (profiling) their counting kernel, of the last call
    else if (!std::strcmp(name, "sparse_sided_items")) *out = (int64_t)c->pp.sided_items;  // those of them the sided route planned (plan.h, Tuning::sparse_sided) ...
    else if (!std::strcmp(name, "sparse_transposed_items")) *out = (int64_t)c->pp.transposed_items;  // ... with the lists on the column block ...
    else if (!std::strcmp(name, "sparse_slabs")) *out = (int64_t)c->pp.slabs.size();  // (block, plane) tables and lists the last dist call's items read
    else if (!std::strcmp(name, "sparse_table_slabs")) *out = (int64_t)c->pp.table_slabs;  // ... and the slabs of the last call built without lists
    else if (!std::strcmp(name, "sparse_table_fills")) {  // table words the LDS placement staged in the last call's launches (plan.h)
        uint64_t f = 0;
        if (c->sparse_run_used)
            for (const auto &rg : c->pp.band_sp_items) f += plan::sparse_table_fills(c->pp.sp_items.data() + rg.first, rg.second - rg.first, c->sparse_run_used);
        *out = (int64_t)f;
    }
    else if (!std::strcmp(name, "sparse_run")) *out = c->sparse_run > 0 ? c->sparse_run : (int64_t)plan::kSparseRunDefault;  // (in effect)
    else if (!std::strcmp(name, "sparse_words")) *out = sparse_words_of(c);  // (in effect; 0: the table is gathered)
    else if (!std::strcmp(name, "sparse_planes")) *out = c->sparse_planes;
    else if (!std::strcmp(name, "sparse_sided")) *out = c->sparse_sided;
    else if (!std::strcmp(name, "sparse_cap")) *out = c->sparse_cap;
    else if (!std::strcmp(name, "words_per_plane")) *out = c->W;
    else if (!std::strcmp(name, "avg_tile_planes_x100")) {
        uint64_t tot = 0;
        for (const auto &t : c->pp.T) tot += t.w - t.z;
        *out = c->pp.T.empty() ? 0 : (int64_t)(tot * 100 / c->pp.T.size());
    }
    else return fail(c, DSH_EINVAL, "unknown info %s", name);
    return DSH_OK;
}

}  // extern "C"

// the plain integer options: a value in [lo, hi] goes to its member, anything else is refused with "<name> <range>"
struct IntOption {
    const char *name;
    int64_t lo, hi;
    const char *range;
    void (*set)(dsh_ctx *c, int64_t v);
};
#define OPT_TO(member, T) [](dsh_ctx *c, int64_t v) { c->member = (T)v; }
static_assert(kGreedyMaxRows == 8192 && plan::kSparseCapMax == 2040 && plan::kSparseRunMax == 65536, "the ranges below name these");
static const IntOption kIntOptions[] = {
    {"cum_budget_bytes", 1 << 20, INT64_MAX, "too small", OPT_TO(cum_budget, uint64_t)},
    {"knn_square_budget_bytes", 0, INT64_MAX, "must be >= 0", OPT_TO(knn_square_budget, uint64_t)},
    {"threshold_band_bytes", 4, INT64_MAX, "must be at least 4", OPT_TO(threshold_band_bytes, uint64_t)},
    {"pairs_chunk", 1, 1 << 24, "must be in [1, 2^24]", OPT_TO(pairs.chunk, uint64_t)},
    {"cluster_chunk", 1, 1 << 26, "must be in [1, 2^26]", OPT_TO(cc.chunk, uint64_t)},
    {"stats_route", -1, 1, "must be -1 (auto), 0 (dense) or 1 (pairs)", OPT_TO(gs.route, int)},
    {"linkage_route", -1, 1, "must be -1 (auto), 0 (dense) or 1 (pairs)", OPT_TO(lk.route, int)},
    {"linkage_partition", 0, 1, "must be 0 or 1", OPT_TO(lk.partition, int)},
    {"linkage_budget_bytes", 64, INT64_MAX, "must be at least 64", OPT_TO(lk.budget, uint64_t)},
    // 6144 members x 24 bytes + the reduction's 6 KiB = 150 KiB of the 160 KiB of LDS
    {"linkage_lds_max", 0, 6144, "must be in [0, 6144]", OPT_TO(lk.lds_max, uint32_t)},
    {"greedy_band_rows", 1, kGreedyMaxRows, "must be in [1, 8192]", OPT_TO(gr.band_rows, uint64_t)},
    {"derive_chunk_bytes", 1, INT64_MAX, "must be at least 1", OPT_TO(derive.chunk_bytes, uint64_t)},
    {"curve_segment", 0, INT64_MAX, "must be >= 0 (0 = the planner's)", OPT_TO(curve.segment, uint64_t)},
    {"curve_scratch_bytes", 1, INT64_MAX, "must be at least 1", OPT_TO(curve.scratch_bytes, uint64_t)},
    {"sort", -1, 1, "must be -1, 0 or 1", OPT_TO(sort_mode, int)},
    {"nsplit", 0, 64, "must be in [0,64]", OPT_TO(nsplit, int)},
    {"part_band_tiles", 1, 1 << 30, "out of range", OPT_TO(part_band_tiles, int)},
    {"xch_tail_bands", 0, 8, "out of range", OPT_TO(tail_bands, int)},
    {"overflow_frag_permille", 0, 1000, "out of range", OPT_TO(overflow_frag_permille, int)},
    {"sparse_planes", -1, 2, "is -1 (auto), 0 (off), 1 or 2", OPT_TO(sparse_planes, int)},  // sparse outer planes (plan.h, Tuning)
    {"sparse_sided", -1, 1, "is -1 (auto), 0 (off) or 1 (forced)", OPT_TO(sparse_sided, int)},  // the sided route (plan.h, Tuning)
    {"sparse_lds", 0, 1, "must be 0 or 1", OPT_TO(sparse_lds, int)},
    {"sparse_run", 0, plan::kSparseRunMax, "must be in [0, 65536]", OPT_TO(sparse_run, int)},
    {"sparse_words", 0, 2, "must be 0 (auto), 1 or 2", OPT_TO(sparse_words, int)},
    {"sparse_cap", 0, plan::kSparseCapMax, "must be in [0, 2040]", OPT_TO(sparse_cap, int)},
    {"xch_recv_gate", -1, 1, "is -1 (auto), 0 or 1", OPT_TO(xch.recv_gate, int)},
    {"finalize_signal", -1, 1, "is -1 (auto), 0 or 1", OPT_TO(finalize_signal, int)},
};
#undef OPT_TO

extern "C" int dsh_set_option(dsh_ctx *c, const char *name, int64_t v)
{
    if (!c || !name) return DSH_EINVAL;
    for (const IntOption &o : kIntOptions) {
        if (std::strcmp(name, o.name)) continue;
        if (v < o.lo || v > o.hi) return fail(c, DSH_EINVAL, "%s %s", o.name, o.range);
        o.set(c, v);
        return DSH_OK;
    }
    // the options that do more than store a value
    if (!std::strcmp(name, "kc")) {
        if (v != 0 && v != 16 && v != 32) return fail(c, DSH_EINVAL, "kc must be 0 (auto), 16 or 32");
        c->kc_opt = (int)v;
        c->planes_valid = false;  // Kpad depends on kc (and pair_groups = auto on kc)
        return DSH_OK;
    }
    if (!std::strcmp(name, "pair_groups")) {
        if (v != 0 && v != 2 && v != 3) return fail(c, DSH_EINVAL, "pair_groups must be 0 (auto), 2 or 3");
        c->pair_groups_opt = (int)v;
        c->planes_valid = false;  // three groups force kc = 16: Kpad depends on kc
        return DSH_OK;
    }
    if (!std::strcmp(name, "range_sort_min_rows")) {
        if (v < 1) return fail(c, DSH_EINVAL, "range_sort_min_rows must be >= 1");
        c->range_sort_min_rows = (int)std::min<int64_t>(v, 1 << 30);
        return DSH_OK;
    }
#ifdef DSH_WHATIF_MFMA
    if (!std::strcmp(name, "pair_mfma")) {  // what-if builds only (make WHATIF=1): the north star keeps the matrix cores off this path
        c->pair_mfma = v != 0;
        return DSH_OK;
    }
#endif
    if (!std::strcmp(name, "finalize_stop")) {  // profiling only: results are meaningless while it is set
        if (v < 0 || v > 4) return fail(c, DSH_EINVAL, "finalize_stop must be in [0,4]");
        if (v && !c->profiling) return fail(c, DSH_ESTATE, "finalize_stop needs dsh_set_profiling(ctx, 1)");
        c->finalize_stop = (int)v;
        return DSH_OK;
    }
    if (!std::strcmp(name, "finalize_timing")) {  // profiling only: same results, the stamped instance of k_finalize
        if (v && !c->profiling) return fail(c, DSH_ESTATE, "finalize_timing needs dsh_set_profiling(ctx, 1)");
        c->finalize_timing = v != 0;
        return DSH_OK;
    }
    if (!std::strcmp(name, "emax") || !std::strcmp(name, "elow")) {
        if (v < -1 || v > (int64_t)kMaxListSide) return fail(c, DSH_EINVAL, "%s must be in [-1,%u]", name, kMaxListSide);
        (name[1] == 'm' ? c->emax_opt : c->elow_opt) = (int)v;
        return DSH_OK;
    }
    return fail(c, DSH_EINVAL, "unknown option %s", name);
}
