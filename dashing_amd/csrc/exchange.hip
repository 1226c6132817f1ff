// exchange.hip -- the multi-GPU exchange behind the C-ABI: point-to-point collection of the ranks' spans of dashing's
// packed triangle on one destination rank -- one message per peer (dsh_collect_spans*), pipelined per part
// (dsh_collect_parts_async), or in the rounds of the exchange-aware pair (dsh_exchange_*: exchange_plan.h plans, this file
// acts) --, dsh_dist_collect over either, and the exchange's diagnostics on one GPU.  The communicator and the poster of a
// grouped round are comm.hip's, the kernels kernels_exchange.hip's.
#include <algorithm>
#include <cstring>

#include "ctx.h"
#include "exchange_plan.h"

using namespace dsh;
using xplan::XMode;
using xplan::xmodes;

namespace {

static_assert(sizeof(PlaceEnt) == xplan::kPlaceEntBytes, "the schedule sizes the table upload by the entries");

// the copy stream waits for part q of the last call with parts: for the flag k_finalize writes from inside its launch
// (hipStreamWaitValue32: >= the call's generation) or, where the call marked its parts with events, for the event
int wait_part(dsh_ctx *c, size_t q)
{
    if (c->parts_signalled) {
        if (q >= kSigMaxParts || !c->sig.ptr) return fail(c, DSH_ESTATE, "internal: part %zu has no flag", q);
        HIPCHK(c, hipStreamWaitValue32(c->copy_stream, (uint32_t *)c->sig.ptr + kSigPartFlag + q, c->sig_gen, hipStreamWaitValueGte, 0xFFFFFFFFu));
        return DSH_OK;
    }
    if (q >= c->ev_part.size()) return fail(c, DSH_ESTATE, "internal: part %zu has no event", q);
    HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_part[q], 0));
    return DSH_OK;
}

// THE gate of a rank's messages: where its parts end in its buffer, and the first part the copy stream has not joined yet
struct PartGate {
    std::vector<uint64_t> part_end;
    size_t next_wait = 0;
    // the copy stream joins the completion (a flag k_finalize sets, or an event) of every part up to part i: the parts of a
    // band are final in ALMOST the order of the list
    int upto(dsh_ctx *c, size_t i)
    {
        for (; next_wait <= i; ++next_wait)
            if (int rc = wait_part(c, next_wait)) return rc;
        return DSH_OK;
    }
    // ... up to the part that holds float x of the buffer (xplan::gate_part); ... every part
    int join(dsh_ctx *c, uint64_t x) { return upto(c, xplan::gate_part(part_end, x)); }
    int rest(dsh_ctx *c) { return part_end.empty() ? DSH_OK : upto(c, part_end.size() - 1); }
};

// cnt floats at base + off, sent to / received from `peer` (a missing base is the poster's to report)
GroupOp send_op(const void *base, uint64_t off, uint64_t cnt, int peer) { return {true, base ? (float *)base + off : nullptr, cnt, peer}; }
GroupOp recv_op(void *base, uint64_t off, uint64_t cnt, int peer) { return {false, (float *)base + off, cnt, peer}; }

// Rounds of whole rows on `st`: round q carries part q of every rank (parts[r]: the row boundaries of rank r's parts) -- the
// destination's own part to its place where it was computed elsewhere, then ONE group with the part of every peer, each
// received at its final place (the ranks' row ranges are contiguous spans of the packed triangle: the destination's links
// are busy at once).  gated: `st` first joins this rank's "part q done" (wait_part); the transfer then runs there while the
// ctx stream computes part q + 1.
int collect_row_rounds(dsh_ctx *c, uint64_t n, const std::vector<std::vector<uint64_t>> &parts, bool gated, hipStream_t st, const void *d_local,
                       void *d_final, int dst)
{
    const int world = comm_who(c).world, rank = comm_who(c).rank;
    auto part = [&](int r, size_t q, uint64_t &off, uint64_t &cnt) {  // part q of rank r in the packed triangle (cnt = 0: it has none)
        const bool has = q + 1 < parts[r].size();
        off = has ? dsh_tri_span(n, 0, parts[r][q]) : 0;
        cnt = has ? dsh_tri_span(n, parts[r][q], parts[r][q + 1]) : 0;
    };
    size_t rounds = 0;
    for (const auto &p : parts) rounds = std::max(rounds, p.size() - 1);
    const uint64_t my_off = dsh_tri_span(n, 0, parts[rank][0]);
    std::vector<GroupOp> ops;
    for (size_t q = 0; q < rounds; ++q) {
        uint64_t off, cnt;
        part(rank, q, off, cnt);
        if (gated && q + 1 < parts[rank].size())
            if (int rc = wait_part(c, q)) return rc;
        if (rank == dst && d_local && cnt && (const float *)d_local + (off - my_off) != (float *)d_final + off)  // computed elsewhere
            HIPCHK(c, hipMemcpyAsync((float *)d_final + off, (const float *)d_local + (off - my_off), cnt * sizeof(float), hipMemcpyDeviceToDevice, st));
        if (world == 1) continue;
        ops.clear();
        if (rank != dst && cnt) ops.push_back(send_op(d_local, off - my_off, cnt, dst));
        for (int src = 0; src < world && rank == dst; ++src) {
            part(src, q, off, cnt);
            if (src != dst && cnt) ops.push_back(recv_op(d_final, off, cnt, src));
        }
        if (int rc = post_group(c, st, ops.data(), ops.size())) return rc;
    }
    return DSH_OK;
}

// one message per peer, all of them in one group on the ctx stream: every rank's range as ONE part
int collect_spans(dsh_ctx *c, uint64_t n, const uint64_t *bounds, const void *d_local, void *d_final, int dst)
{
    const CommWho who = comm_who(c);
    int rc = validate_bounds(c, n, bounds, who.world, dst);
    if (rc) return rc;
    if (who.rank == dst ? !d_final : dsh_tri_span(n, bounds[who.rank], bounds[who.rank + 1]) && !d_local) return DSH_EINVAL;
    std::vector<std::vector<uint64_t>> parts((size_t)who.world);
    for (int r = 0; r < who.world; ++r) parts[r] = {bounds[r], bounds[r + 1]};
    return collect_row_rounds(c, n, parts, false, c->stream, d_local, d_final, dst);
}

}  // namespace

extern "C" {

int dsh_collect_spans_async(dsh_ctx *c, uint64_t n, const uint64_t *bounds, const void *d_local, void *d_final, int dst)
{
    if (!c) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    if ((rc = need_comm(c, bounds && bounds[0] == 0 && bounds[1] == n))) return rc;
    return collect_spans(c, n, bounds, d_local, d_final, dst);
}

int dsh_collect_spans(dsh_ctx *c, uint64_t n, const uint64_t *bounds, const void *d_local, void *d_final, int dst)
{
    int rc = dsh_collect_spans_async(c, n, bounds, d_local, d_final, dst);
    if (rc) return rc;
    return sync_guarded(c, c->stream, "dsh_collect_spans");
}

int dsh_collect_parts_async(dsh_ctx *c, uint64_t n, const uint64_t *bounds, uint32_t nparts, const void *d_local,
                            void *d_final, int dst)
{
    if (!c || !bounds || nparts == 0) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    const int world = comm_who(c).world, rank = comm_who(c).rank;
    if ((rc = need_comm(c, bounds[0] == 0 && bounds[1] == n))) return rc;
    if ((rc = validate_bounds(c, n, bounds, world, dst))) return rc;
    if (rank == dst && !d_final) return DSH_EINVAL;
    // every rank's parts, from the same function the compute used (dsh_range_parts): both sides of a message agree.
    // dsh_dist_rows_parts_device_async lays ANY non-empty range out in exactly these parts (a short range: one part) and
    // records an event for each, so a rank with few rows takes part in the rounds like every other.
    std::vector<std::vector<uint64_t>> parts((size_t)world);
    for (int r = 0; r < world; ++r) plan::range_parts(n, bounds[r], bounds[r + 1], nparts, parts[r]);
    const size_t myparts = parts[rank].size() - 1;
    if (c->parts_done != myparts)
        return fail(c, DSH_ESTATE, "dsh_dist_rows_parts_device_async(%u parts) of this rank's rows must come first (%u parts computed, %zu expected)",
                    nparts, c->parts_done, myparts);
    return collect_row_rounds(c, n, parts, true, c->copy_stream, d_local, d_final, dst);
}

}  // extern "C"

/* ---- the exchange-aware pair: every rank's buffer laid out for the exchange (plan.h: row sets, row-sorted parts) ------ */
namespace {

XMode xmode(uint64_t n, const plan::RowSets &rs, int r, uint32_t nparts, int dst) { return xmodes(n, rs, nparts, dst)[(size_t)r]; }

int parse_table(dsh_ctx *c, uint64_t n, const uint64_t *rowsets, int dst, plan::RowSets &rs)
{
    if (const char *why = plan::parse_rowsets(rowsets, n, rs)) return fail(c, DSH_EINVAL, "%s", why);
    if (dst < 0 || (uint32_t)dst >= rs.world) return fail(c, DSH_EINVAL, "bad destination rank %d (world %u)", dst, rs.world);
    return DSH_OK;
}

// every rank's mode as the calling rank's compute call cut them; that call must have come first
int caller_modes(dsh_ctx *c, uint64_t n, const plan::RowSets &rs, uint32_t nparts, int dst, int rank, std::vector<XMode> &modes)
{
    modes = xmodes(n, rs, nparts, dst, c->parts_signalled ? rank : -1);
    if (c->parts_done != modes[(size_t)rank].nparts())
        return fail(c, DSH_ESTATE, "dsh_exchange_rows_device_async of this rank's rows must come first (%u parts computed, %zu expected)",
                    c->parts_done, modes[(size_t)rank].nparts());
    return DSH_OK;
}

// the key order and the row offsets of a rank's row-sorted buffer (xplan::rowsorted_tables) from THIS context's host copy of
// the keys
int rowsorted_tables(dsh_ctx *c, uint64_t n, const XMode &m, std::vector<uint32_t> &order, std::vector<uint64_t> &rowoff)
{
    if (!c->hk32_valid || c->card_from > m.rb)
        return fail(c, DSH_ESTATE, "the per-sketch pass of this context does not cover the rows from %llu on (compute this rank's rows first)",
                    (unsigned long long)m.rb);
    xplan::rowsorted_tables(c->hk32, n, m, order, rowoff, c->lay.sort_a);
    return DSH_OK;
}

// the destination's own rows, computed relative to its first row: every segment of them to its place in the final matrix
// (a no-op when they were computed in place)
int place_own_rows(dsh_ctx *c, uint64_t n, const XMode &m, const void *d_local, void *d_final, hipStream_t st)
{
    const uint64_t base = dsh_tri_span(n, 0, m.rb);
    if (!d_local || (const float *)d_local == (float *)d_final + base) return DSH_OK;
    auto seg = [&](uint64_t b, uint64_t e) -> int {
        const uint64_t off = dsh_tri_span(n, 0, b), cnt = dsh_tri_span(n, b, e);
        if (cnt)
            HIPCHK(c, hipMemcpyAsync((float *)d_final + off, (const float *)d_local + (off - base), cnt * sizeof(float), hipMemcpyDeviceToDevice, st));
        return DSH_OK;
    };
    int rc = seg(m.rb, m.re);
    for (size_t x = 0; !rc && x + 1 < m.extra.size(); x += 2) rc = seg(m.extra[x], m.extra[x + 1]);
    return rc;
}

}  // namespace

extern "C" {

int dsh_exchange_mode(uint64_t n, const uint64_t *rowsets, int rank, uint32_t nparts, int dst, int *rowsorted, uint32_t *nparts_out,
                      uint64_t *local_floats_out)
{
    plan::RowSets rs;
    if (nparts == 0 || plan::parse_rowsets(rowsets, n, rs) || rank < 0 || (uint32_t)rank >= rs.world || dst < 0 || (uint32_t)dst >= rs.world)
        return DSH_EINVAL;
    const XMode m = xmode(n, rs, rank, nparts, dst);
    if (rowsorted) *rowsorted = m.rowsorted ? 1 : 0;
    if (nparts_out) *nparts_out = (uint32_t)m.nparts();
    if (local_floats_out) {
        // the destination computes relative to its first row (in place in the final matrix, or a buffer that reaches to
        // the end of its last segment); every other rank's buffer holds exactly its rows
        if (m.rb >= m.re) *local_floats_out = 0;
        else if (rank == dst) *local_floats_out = dsh_tri_span(n, m.rb, m.extra.empty() ? m.re : m.extra.back());
        else *local_floats_out = m.span(n);
    }
    return DSH_OK;
}

int dsh_exchange_rows_device_async(dsh_ctx *c, int estim, int result_type, int k, const uint64_t *rowsets, int rank, uint32_t nparts,
                                   int dst, void *d_local)
{
    if (!c || !rowsets || nparts == 0 || rank < 0) return DSH_EINVAL;
    int rc = enter(c);
    if (rc) return rc;
    plan::RowSets rs;
    if ((rc = parse_table(c, c->n, rowsets, dst, rs))) return rc;
    if ((uint32_t)rank >= rs.world) return fail(c, DSH_EINVAL, "bad rank %d (world %u)", rank, rs.world);
    reset_prof(c);
    c->parts_done = 0;
    if (c->n < 2) return DSH_OK;
    const std::vector<XMode> modes = xmodes(c->n, rs, nparts, dst, parts_will_signal(c) ? rank : -1);
    const XMode &m = modes[(size_t)rank];
    // the destination places the row-sorted spans of the others: its per-sketch pass must cover their rows too -- also
    // when it holds no rows itself (it used to return before any pass and fail later in the collect, with the
    // peers' sends already posted)
    bool from_zero = false;
    uint64_t first_needed = m.rb < m.re ? m.rb : c->n;
    if (rank == dst)
        for (uint32_t r = 0; r < rs.world; ++r) {
            if ((int)r == dst) continue;
            const XMode &o = modes[r];
            if (o.rowsorted && o.rb < first_needed) from_zero = true;
        }
    if (m.rb >= m.re) {
        if (!from_zero) return DSH_OK;
        c->pass_from_zero = true;
        rc = prepare(c, estim, -1, /*card_only=*/true);
        c->pass_from_zero = false;
        if (rc) return rc;
        if (!c->hk32_valid) {  // (a cardinality pass does not wait for its keys: the collect's tables need them)
            HIPCHK(c, hipEventSynchronize(c->ev_keys));
            c->hk32_valid = true;
        }
        return DSH_OK;
    }
    if (!d_local) return DSH_EINVAL;
    c->pass_from_zero = from_zero;
    PairJob j = PairJob::triangle(estim, result_type, k, m.rb, m.re, dsh_tri_span(c->n, 0, m.rb), d_local);
    j.nparts = rank == dst ? 1 : m.kreq;
    j.rowsorted = m.rowsorted ? 1 : 0;
    j.extra = m.extra;
    rc = run_pairs(c, j);
    c->pass_from_zero = false;
    return rc;
}

}  // extern "C"

/* ---- dsh_exchange_collect_async: the phases of a call over the one struct they share ---------------------------------- */
namespace {

struct Collect {
    uint64_t n;
    uint32_t nparts;
    const void *d_local;
    void *d_final;
    int dst;
    CommWho who;
    plan::RowSets rs;
    std::vector<XMode> modes;                   // (as this rank's compute call cut them)
    // row-sorted sources: their key order and row offsets.  A source knows its own (the layout); the destination derives
    // them from its keys
    std::vector<std::vector<uint64_t>> rowoff;
    std::vector<std::vector<uint32_t>> order;
    xplan::Schedule S;
    PartGate gate;                              // (source) of this rank's messages
    bool placed = false;
    bool is_dst() const { return who.rank == dst; }
    const XMode &mine() const { return modes[(size_t)who.rank]; }
};

int collect_validate(dsh_ctx *c, const uint64_t *rowsets, Collect &X)
{
    int rc = parse_table(c, X.n, rowsets, X.dst, X.rs);
    if (rc) return rc;
    X.who = comm_who(c);
    if ((rc = need_comm(c, X.rs.world == 1))) return rc;
    if ((int)X.rs.world != X.who.world)
        return fail(c, DSH_EINVAL, "the row-set table is for %u ranks, the communicator has %d", X.rs.world, X.who.world);
    if (X.is_dst() && !X.d_final) return DSH_EINVAL;
    return DSH_OK;
}

int collect_plan(dsh_ctx *c, Collect &X)
{
    const int world = X.who.world, rank = X.who.rank;
    if (int rc = caller_modes(c, X.n, X.rs, X.nparts, X.dst, rank, X.modes)) return rc;
    X.rowoff.resize((size_t)world), X.order.resize((size_t)world);
    if (!X.is_dst()) {
        if (X.mine().rowsorted) X.rowoff[rank] = c->lay.rowoff_w;
    } else {
        for (int r = 0; r < world; ++r)
            if (r != X.dst && X.modes[r].rowsorted)
                if (int rc = rowsorted_tables(c, X.n, X.modes[r], X.order[r], X.rowoff[r])) return rc;
    }
    X.S = xplan::schedule(X.n, X.modes, X.nparts, X.dst, rank, X.rowoff);
    X.gate.part_end = X.S.part_end;
    return DSH_OK;
}

// destination: the buffers, the pinned tables, the entries' device addresses, the upload (on the copy stream, in front of
// the first receive)
int collect_upload(dsh_ctx *c, Collect &X)
{
    const xplan::Schedule &S = X.S;
    if (!X.is_dst() || !S.stage_total) return DSH_OK;
    HIPCHK(c, c->xch.stage.ensure(S.stage_total * sizeof(float)));
    HIPCHK(c, c->xch.tabs.wait());  // the previous call's upload from the pinned tables
    HIPCHK(c, c->xch.tabs.room(S.tab_bytes));
    HIPCHK(c, c->xch.tab.ensure(S.tab_bytes));
    uint8_t *const host = (uint8_t *)c->xch.tabs.ptr();
    for (int r = 0; r < X.who.world; ++r) {
        if (r == X.dst || !X.modes[r].rowsorted) continue;
        uint8_t *h = host + S.tab_off[r];
        std::memcpy(h, X.rowoff[r].data(), X.rowoff[r].size() * sizeof(uint64_t));
        std::memcpy(h + X.rowoff[r].size() * sizeof(uint64_t), X.order[r].data(), X.order[r].size() * sizeof(uint32_t));
    }
    PlaceEnt *ents = (PlaceEnt *)(host + S.ent_off);
    for (size_t x = 0; x < S.ents.size(); ++x) {
        const xplan::Ent &e = S.ents[x];
        const uint8_t *t = (const uint8_t *)c->xch.tab.ptr + S.tab_off[e.src];
        ents[x].src = (const float *)c->xch.stage.ptr + S.stage_off[e.src];
        ents[x].order = (const uint32_t *)(t + X.rowoff[e.src].size() * sizeof(uint64_t));
        ents[x].rowoff = (const uint64_t *)t;
        ents[x].pos0 = e.pos0, ents[x].row0 = e.row0, ents[x].nrows = e.nrows;
    }
    HIPCHK(c, hipMemcpyAsync(c->xch.tab.ptr, host, S.tab_bytes, hipMemcpyHostToDevice, c->copy_stream));
    HIPCHK(c, c->xch.tabs.sent(c->copy_stream));
    while (c->xch.ev_round.size() < S.M) HIPCHK(c, add_event(c->xch.ev_round));
    return DSH_OK;
}

// The destination's receives: an RCCL kernel that waits for its peers spins on the GPU; beside the phase-locked tile
// kernel it would slow every round down to the CU it shares.  A SHORT job of the destination (one launch of at most 8
// rounds: its peers then run 6 + 1 rounds and have nothing to send before about the same moment) therefore posts its
// receives behind its tile kernel; longer jobs post at once -- their peers' first messages come much earlier (option
// xch_recv_gate: -1 auto | 0 at once | 1 behind the first tile kernel).
int collect_recv_gate(dsh_ctx *c, Collect &X)
{
    if (!(X.is_dst() && X.who.world > 1 && X.mine().nparts() && c->ev_first_tiles)) return DSH_OK;
    const uint64_t rounds = (c->pp.items.size() + 511) / 512;
    const bool gate = c->xch.recv_gate == 1 || (c->xch.recv_gate < 0 && c->last_bands == 1 && rounds <= 8);
    if (gate) HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->ev_first_tiles, 0));
    c->xch.recv_gated = gate;
    return DSH_OK;
}

// the rounds: message q of every source in one grouped call on the copy stream -- a source's behind the gate of the part
// that holds its last value --, and behind it the destination's placement of the rows that are now complete
int collect_rounds(dsh_ctx *c, Collect &X)
{
    const xplan::Schedule &S = X.S;
    std::vector<GroupOp> ops;
    for (size_t q = 0; q < S.M && X.who.world > 1; ++q) {
        if (!S.post[q]) continue;
        ops.clear();
        if (X.is_dst()) {
            for (int src = 0; src < X.who.world; ++src) {
                const xplan::Msg &m = S.msg(q, src);
                if (src == X.dst || !m.cnt) continue;
                if (X.modes[src].rowsorted) ops.push_back(recv_op(c->xch.stage.ptr, S.stage_off[src] + m.first, m.cnt, src));
                else ops.push_back(recv_op(X.d_final, dsh_tri_span(X.n, 0, X.modes[src].rb) + m.first, m.cnt, src));
            }
        } else {
            if (int rc = X.gate.upto(c, S.gate[q])) return rc;
            ops.push_back(send_op(X.d_local, S.msg(q, X.who.rank).first, S.msg(q, X.who.rank).cnt, X.dst));
        }
        if (int rc = post_group(c, c->copy_stream, ops.data(), ops.size())) return rc;
        // the rows that are now complete go to their places: ONE launch per round, on a stream of its own behind the
        // round's event, so that the next round's transfer does not wait for it
        if (X.is_dst() && S.stage_total && S.round_rows[q]) {
            HIPCHK(c, hipEventRecord(c->xch.ev_round[q], c->copy_stream));
            HIPCHK(c, hipStreamWaitEvent(c->place_stream, c->xch.ev_round[q], 0));
            HIPCHK(c, launch_rows_place(c->place_stream, (const PlaceEnt *)((const uint8_t *)c->xch.tab.ptr + S.ent_off) + S.round_ent[q],
                                        S.round_ent[q + 1] - S.round_ent[q], S.round_rows[q], (float *)X.d_final, X.n));
            X.placed = true;
        }
    }
    return DSH_OK;
}

// the destination's own rows (one part, normally computed in place) and the placements: the copy stream, which
// dsh_comm_wait waits for, ends behind both
int collect_close(dsh_ctx *c, Collect &X)
{
    if (!X.is_dst()) return DSH_OK;
    if (X.mine().nparts()) {
        int rc = wait_part(c, 0);
        if (rc) return rc;
        if ((rc = place_own_rows(c, X.n, X.mine(), X.d_local, X.d_final, c->copy_stream))) return rc;
    }
    if (X.placed) {
        HIPCHK(c, c->xch.ev_place_done.ensure());
        HIPCHK(c, hipEventRecord(c->xch.ev_place_done, c->place_stream));
        HIPCHK(c, hipStreamWaitEvent(c->copy_stream, c->xch.ev_place_done, 0));
    }
    return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_exchange_collect_async(dsh_ctx *c, uint64_t n, const uint64_t *rowsets, uint32_t nparts, const void *d_local, void *d_final,
                               int dst)
{
    if (!c || !rowsets || nparts == 0) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    Collect X{n, nparts, d_local, d_final, dst};
    if ((rc = collect_validate(c, rowsets, X))) return rc;
    if (n < 2) return DSH_OK;  // (dsh_exchange_rows_device_async computed nothing either: no pairs, no messages)
    if ((rc = collect_plan(c, X))) return rc;
    if ((rc = collect_upload(c, X))) return rc;
    if ((rc = collect_recv_gate(c, X))) return rc;
    if ((rc = collect_rounds(c, X))) return rc;
    return collect_close(c, X);
}

int dsh_exchange_place_device(dsh_ctx *c, const uint64_t *rowsets, int src, uint32_t nparts, int dst, const void *d_src_local,
                              void *d_final)
{
    if (!c || !rowsets || nparts == 0 || src < 0 || !d_final) return DSH_EINVAL;
    int rc = enter(c);
    if (rc) return rc;
    const uint64_t n = c->n;
    plan::RowSets rs;
    if ((rc = parse_table(c, n, rowsets, dst, rs))) return rc;
    if ((uint32_t)src >= rs.world) return fail(c, DSH_EINVAL, "bad source rank %d (world %u)", src, rs.world);
    const XMode m = xmode(n, rs, src, nparts, dst);
    if (!m.span(n)) return DSH_OK;
    if (!d_src_local) return DSH_EINVAL;
    // (its own table buffer, on the ctx stream: dsh_exchange_collect_async keeps xch_tab busy on the copy stream -- ADVICE r4)
    if (!m.rowsorted) {  // final order already (relative to the rank's first row): every segment goes to its place
        if ((rc = place_own_rows(c, n, m, d_src_local, d_final, c->stream))) return rc;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return DSH_OK;
    }
    std::vector<uint32_t> order;
    std::vector<uint64_t> rowoff;
    if ((rc = rowsorted_tables(c, n, m, order, rowoff))) return rc;
    const size_t ro_bytes = rowoff.size() * sizeof(uint64_t), bytes = ro_bytes + order.size() * sizeof(uint32_t);
    HIPCHK(c, c->xch.place_tab.ensure(bytes));
    HIPCHK(c, hipMemcpyAsync(c->xch.place_tab.ptr, rowoff.data(), ro_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync((uint8_t *)c->xch.place_tab.ptr + ro_bytes, order.data(), order.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    if (c->profiling) c->ev_used = 0;  // (no other timer of this call holds an event of the pool)
    DeviceTimer t(c, c->stream);  // (profiling: the device time of the placement itself, dsh_get_info "place_kernel_us")
    HIPCHK(c, launch_row_place(c->stream, (const float *)d_src_local, (float *)d_final,
                               (const uint32_t *)((const uint8_t *)c->xch.place_tab.ptr + ro_bytes), (const uint64_t *)c->xch.place_tab.ptr,
                               0, order.size(), n));
    t.stop(c->xch.place_ms);
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the pageable tables must outlive their copies)
    return DSH_OK;
}

/* ---- diagnostics of the exchange on ONE GPU (no communicator needed; the kernels: kernels_exchange.hip) --------------- */
int dsh_exchange_probe_parts_async(dsh_ctx *c, uint64_t n, const uint64_t *rowsets, int rank, uint32_t nparts, int dst,
                                   const void *d_local, void *d_probe)
{
    if (!c || !rowsets || nparts == 0 || rank < 0 || !d_local || !d_probe) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    plan::RowSets rs;
    if ((rc = parse_table(c, n, rowsets, dst, rs))) return rc;
    if ((uint32_t)rank >= rs.world) return fail(c, DSH_EINVAL, "bad rank %d (world %u)", rank, rs.world);
    std::vector<XMode> modes;
    if ((rc = caller_modes(c, n, rs, nparts, dst, rank, modes))) return rc;
    const XMode &mine = modes[(size_t)rank];
    // where the parts end in the rank's buffer (the destination computes relative to its first row, as one part)
    PartGate gate{xplan::part_ends(n, mine, c->lay.rowoff_w, rank == dst)};
    const std::vector<uint64_t> &part_end = gate.part_end;
    if (c->xch.comm && c->xch.world == 1) {
        // The reader is librccl itself: the rank's step as dsh_exchange_collect_async runs it for a source -- M = nparts
        // rounds, message q of the buffer behind the gate of the part that holds its last value, one grouped call per round
        // -- with the one peer a communicator of one rank has: ncclSend to itself paired with the ncclRecv into d_probe.
        const uint64_t total = part_end.empty() ? 0 : part_end.back();
        const size_t M = nparts;
        for (size_t q = 0; q < M && total; ++q) {
            uint64_t first, cnt;
            xplan::message_span(total, q, M, first, cnt);
            if (!cnt) continue;
            if ((rc = gate.join(c, first + cnt))) return rc;
            const GroupOp ops[2] = {send_op(d_local, first, cnt, 0), recv_op(d_probe, first, cnt, 0)};
            if ((rc = post_group(c, c->copy_stream, ops, 2))) return rc;
        }
        return gate.rest(c);  // (every gate is joined, as in the kernel-reader path)
    }
    uint64_t at = 0;
    for (size_t i = 0; i < part_end.size(); ++i) {
        const uint64_t end = part_end[i];
        if ((rc = gate.upto(c, i))) return rc;
        if (end > at) HIPCHK(c, launch_probe_copy(c->copy_stream, (const float *)d_local + at, (float *)d_probe + at, end - at));
        at = end;
    }
    return DSH_OK;
}

int dsh_diag_spin_start(dsh_ctx *c, uint32_t nblocks, uint32_t threads, uint32_t lds_bytes, uint32_t max_ms)
{
    if (!c || nblocks == 0 || nblocks > 4096 || threads < 64 || threads > 1024 || (threads & 63) || lds_bytes > 160 * 1024 || max_ms == 0 || max_ms > 10000)
        return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    if (c->xch.spin_running) return fail(c, DSH_ESTATE, "dsh_diag_spin_stop first");
    (void)device_can_wait_value(c);  // (also asks for the wall clock's rate)
    if (c->wall_clock_khz <= 0) return fail(c, DSH_ENODEV, "the device reports no wall clock rate");
    HIPCHK(c, c->xch.spin_flag.ensure());
    HIPCHK(c, c->spin_stream.create());
    *(volatile uint32_t *)c->xch.spin_flag.ptr = 0;
    uint32_t *dflag = nullptr;
    HIPCHK(c, hipHostGetDevicePointer((void **)&dflag, c->xch.spin_flag.ptr, 0));
    HIPCHK(c, launch_diag_spin(c->spin_stream, nblocks, threads, lds_bytes, dflag, (unsigned long long)max_ms * (unsigned long long)c->wall_clock_khz));
    c->xch.spin_running = true;
    return DSH_OK;
}

int dsh_diag_spin_stop(dsh_ctx *c)
{
    if (!c) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    if (!c->xch.spin_running) return DSH_OK;
    *(volatile uint32_t *)c->xch.spin_flag.ptr = 1;
    c->xch.spin_running = false;
    HIPCHK(c, hipStreamSynchronize(c->spin_stream));
    return DSH_OK;
}

}  // extern "C"

namespace {

// dsh_dist_collect's buffers: the destination assembles the matrix in gather_full and computes its own rows in place, at
// the offset of its first row; every other rank computes into gather_local
int collect_buffer(dsh_ctx *c, bool is_dst, uint64_t total, uint64_t own_off, uint64_t local_floats, const float *out, void *&d_loc)
{
    if (is_dst) {
        if (total && !out) return DSH_EINVAL;
        HIPCHK(c, c->xch.gather_full.ensure(std::max<uint64_t>(total, 1) * sizeof(float)));
        d_loc = (float *)c->xch.gather_full.ptr + own_off;
    } else {
        HIPCHK(c, c->xch.gather_local.ensure(std::max<uint64_t>(local_floats, 1) * sizeof(float)));
        d_loc = c->xch.gather_local.ptr;
    }
    return DSH_OK;
}

// ... and the destination's download of the assembled matrix
int collect_download(dsh_ctx *c, bool is_dst, uint64_t total, float *out)
{
    if (is_dst && total)
        HIPCHK(c, hipMemcpyAsync(out, c->xch.gather_full.ptr, total * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    return sync_guarded(c, c->stream, "dsh_dist_collect");
}

}  // namespace

extern "C" {

int dsh_dist_collect(dsh_ctx *c, int estim, int result_type, int k, const uint64_t *bounds, int dst, float *out)
{
    int rc = enter(c);
    if (rc) return rc;
    const int world = comm_who(c).world, rank = comm_who(c).rank;
    const uint64_t n = c->n, total = dsh_tri_span(n, 0, n);
    void *d_loc = nullptr;
    if (!bounds) {
        // the library's own partition: balanced row sets (range + top-up tile rows, dsh_balance_rowsets) through the
        // pipelined exchange pair -- what bench.py --gpus N times, for a host without device pointers
        if (dst < 0 || dst >= world) return fail(c, DSH_EINVAL, "bad destination rank %d (world %d)", dst, world);
        if (n < 2) return DSH_OK;  // no pairs: an empty matrix on every rank, nothing to exchange
        plan::RowSets rs;
        plan::balance_rowsets(n, (uint32_t)world, rs, ~0u, dst);
        std::vector<uint64_t> tab(rs.words());
        rs.write(tab.data());
        constexpr uint32_t kParts = 8;
        uint64_t local_floats = 0;
        if ((rc = dsh_exchange_mode(n, tab.data(), rank, kParts, dst, nullptr, nullptr, &local_floats))) return fail(c, rc, "internal: row-set table");
        uint64_t rb = 0, re = 0;
        std::vector<uint64_t> ex;
        rs.rank_rows((uint32_t)rank, rb, re, ex);
        if ((rc = collect_buffer(c, rank == dst, total, dsh_tri_span(n, 0, rb), local_floats, out, d_loc))) return rc;
        if ((rc = dsh_exchange_rows_device_async(c, estim, result_type, k, tab.data(), rank, kParts, dst, d_loc))) return rc;
        if ((rc = dsh_exchange_collect_async(c, n, tab.data(), kParts, rank == dst ? nullptr : d_loc, rank == dst ? c->xch.gather_full.ptr : nullptr, dst)))
            return rc;
        if ((rc = sync_guarded(c, c->stream, "dsh_dist_collect (ctx stream)"))) return rc;
        if ((rc = sync_guarded(c, c->copy_stream, "dsh_dist_collect (copy stream)"))) return rc;
        return collect_download(c, rank == dst, total, out);
    }
    if ((rc = validate_bounds(c, n, bounds, world, dst))) return rc;  // before anything is sized by them
    const uint64_t mine = dsh_tri_span(n, bounds[rank], bounds[rank + 1]);
    if ((rc = collect_buffer(c, rank == dst, total, dsh_tri_span(n, 0, bounds[rank]), mine, out, d_loc))) return rc;
    if (mine && (rc = dsh_dist_rows_device_async(c, estim, result_type, k, bounds[rank], bounds[rank + 1], d_loc))) return rc;
    if ((rc = collect_spans(c, n, bounds, d_loc, rank == dst ? c->xch.gather_full.ptr : nullptr, dst))) return rc;
    return collect_download(c, rank == dst, total, out);
}

}  // extern "C"
