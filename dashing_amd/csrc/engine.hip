// engine.hip -- the device side of a compare pass: prepare() builds what a layout needs (per-sketch pass, key-ordered
// columns, bit-planes, position index), run_pairs() launches the tile kernel and k_finalize over the plan of plan.cpp.
// Together they replace dist_loop / perform_core_op (src/sketch_and_cmp.h:785-880, :699-710) and the compare side of
// dm::parallel_fill (distmat/distmat.h:459-512).
#include <algorithm>
#include <chrono>
#include <cstring>

#include "ctx.h"

namespace dsh {

int prepare(dsh_ctx *c, int estim, int want_sorted, bool card_only, uint64_t want_rb, uint64_t want_re, uint32_t nparts,
            int rowsorted, const std::vector<uint64_t> *extra_in)
{
    static const std::vector<uint64_t> kNoExtra;
    std::vector<uint64_t> extra_cached;
    const std::vector<uint64_t> *extra = extra_in ? extra_in : &kNoExtra;
    if (!c->have_sketches) return fail(c, DSH_ESTATE, "no sketches loaded");
    if (estim < 0 || estim > 2) return fail(c, DSH_EINVAL, "bad estimator %d", estim);
    if (want_sorted < 0) {  // "whatever is cached"
        want_sorted = c->lay.sorted;
        want_rb = c->lay.rb;
        want_re = c->lay.re;
        rowsorted = 0;
        extra_cached = c->lay.extra;
        extra = &extra_cached;
    }
    if (!want_sorted) rowsorted = 0, extra = &kNoExtra;
    if (want_re > c->n) want_re = c->n;
    if (!want_sorted) want_rb = 0, want_re = c->n;
    if (want_rb > want_re) want_rb = want_re;
    const uint64_t n = c->n;
    std::vector<uint64_t> parts, rs_pos;
    if (want_rb >= want_re) extra = &kNoExtra;
    if (want_sorted && !rowsorted) {
        if (extra->empty()) plan::range_parts(n, want_rb, want_re, std::max<uint32_t>(nparts, 1), parts);
        else parts = {want_rb, want_re};  // (a range with extra segments is ONE part)
    }
    if (rowsorted) plan::rowsorted_part_positions(n, want_rb, want_re, std::max<uint32_t>(nparts, 1), rs_pos, extra);
    const int emax_new = c->emax_opt >= 0 ? std::min<int>(c->emax_opt, (int)kMaxListSide) : plan::auto_list_cap(c->p, true);
    const int elow_new = c->elow_opt >= 0 ? std::min<int>(c->elow_opt, (int)kMaxListSide) : plan::auto_list_cap(c->p, false);
    if (emax_new != c->emax || elow_new != c->elow) {  // thresholds and lists (hence planes) depend on them
        c->planes_valid = false;
        c->card_estim = -1;
    }
    c->emax = emax_new;
    c->elow = elow_new;
    // (the layout keeps cardinalities, keys and lists per column: it is only "the same" while it was built from the
    // per-sketch pass that is current -- another estimator or other list caps start a new pass)
    const bool same_layout = c->planes_valid && c->lay_gen == c->pass_gen && c->lay.sorted == want_sorted &&
                             (!want_sorted || (c->lay.rb == want_rb && c->lay.re == want_re && c->lay.rowsorted == rowsorted &&
                                               c->lay.extra == *extra && (rowsorted ? c->lay.part_w == rs_pos : c->lay.parts == parts)));
    // sketches the per-sketch pass has to cover: a row range of the triangle never looks at the sketches before it
    const uint64_t need_from = (card_only || !want_sorted || c->pass_from_zero) ? 0 : want_rb;
    const bool have_pass = c->card_estim == estim && c->card_from <= need_from;
    if (have_pass && (card_only || same_layout)) return DSH_OK;
    const bool keep_layout = same_layout && have_pass;  // (a new pass below also outdates the layout's per-column data)
    DeviceTimer timer(c, c->stream);
    // the per-sketch pass depends on (registers, estimator, emax) only: a new column layout reuses it
    if (!have_pass) {
        HIPCHK(c, c->card.ensure(std::max<uint64_t>(n, 1) * sizeof(double)));
        HIPCHK(c, c->exc.ensure(std::max<uint64_t>(n, 1) * kListCap * (c->p <= 15 ? 2 : 4)));
        HIPCHK(c, c->excv.ensure(std::max<uint64_t>(n, 1) * kListCap));
        HIPCHK(c, c->exc_n.ensure(std::max<uint64_t>(n, 1) * sizeof(uint32_t)));
        // (keys [n], then the counts [n] and the thresholds [n] of the sparse-plane planner: one buffer, one transfer)
        HIPCHK(c, c->keys.ensure(std::max<uint64_t>(n, 1) * 3 * sizeof(uint32_t)));
        HIPCHK(c, c->tailhist.ensure(std::max<uint64_t>(n, 1) * 64));
        HIPCHK(c, c->hist.ensure(std::max<uint64_t>(n, 1) * 64 * sizeof(uint32_t)));
        HIPCHK(c, launch_selfhist_card(c->stream, c->regs, need_from, n, c->p, estim, c->emax, c->elow,
                                       (uint32_t *)c->hist.ptr, c->exc.ptr, (uint8_t *)c->excv.ptr,
                                       (uint32_t *)c->exc_n.ptr, (uint32_t *)c->keys.ptr,
                                       (uint8_t *)c->tailhist.ptr, (uint32_t *)c->keys.ptr + n, (uint32_t *)c->keys.ptr + 2 * n,
                                       std::min<uint32_t>((uint32_t)c->sparse_cap, plan::kSparseCapMax)));
        c->pass_sparse_cap = std::min<uint32_t>((uint32_t)c->sparse_cap, plan::kSparseCapMax);
        // the keys travel to the host right behind the per-sketch pass (the column order is made there); the
        // cardinalities follow on the stream while the host sorts
        HIPCHK(c, c->pin_keys.ensure(std::max<uint64_t>(n, 1) * 3 * sizeof(uint32_t)));
        c->hk32 = (const uint32_t *)c->pin_keys.ptr;
        c->hg32 = c->hk32 + n;
        c->hv32 = c->hk32 + 2 * n;
        if (n > need_from)  // (the keys from need_from on and every count: the counts in front of need_from are never read)
            HIPCHK(c, hipMemcpyAsync((uint32_t *)c->pin_keys.ptr + need_from, (const uint32_t *)c->keys.ptr + need_from,
                                     (3 * n - need_from) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, c->ev_keys.ensure());
        HIPCHK(c, hipEventRecord(c->ev_keys, c->stream));
        HIPCHK(c, launch_card_from_hist(c->stream, (const uint32_t *)c->hist.ptr, (const uint32_t *)c->keys.ptr, need_from, n,
                                        c->p, estim, (double *)c->card.ptr));
        c->card_estim = estim;
        c->card_from = need_from;
        c->hk32_valid = false;
        ++c->pass_gen;
    }
    if (card_only) {  // a cardinality query never builds planes (and leaves stale ones marked so)
        timer.stop(c->prep_ms, /*add=*/true);
        return DSH_OK;
    }
#ifdef DSH_EXPERIMENT_REUSE_LAYOUT
    // EXPERIMENT (make EXPERIMENT=1; never in the product library): the upper bound of what ANY device-built layout could
    // save.  The sketches of a re-attached matrix are the same bytes, so the layout of the previous call -- host tables AND
    // the permutation on the device -- is still right: skip the host's part entirely (the wait for the keys, the radix sort,
    // the block statistics, the uploads) and go straight from the per-sketch pass to the index build and the transform.
    // Results stay correct only while every call sees the same registers (bench.py's timed loop).  DESIGN.md section 8.
    const bool reuse_host_layout = !keep_layout && c->lay_built && c->lay.n == n && c->lay.sorted == want_sorted &&
                                   (!want_sorted || (c->lay.rb == want_rb && c->lay.re == want_re && c->lay.rowsorted == rowsorted &&
                                                     c->lay.extra == *extra && (rowsorted ? c->lay.part_w == rs_pos : c->lay.parts == parts)));
#else
    constexpr bool reuse_host_layout = false;
#endif
    if (!keep_layout) {
        if (c->p > kMaxPCompare)
            return fail(c, DSH_EINVAL, "the compare path takes p <= %d (p=%d: sketching and cardinalities only)", kMaxPCompare, c->p);
        // three items per workgroup exist at 16-row stages only (LDS, kernels.h)
        if (c->pair_groups_opt == 3 && c->kc_opt == 32)
            return fail(c, DSH_EINVAL, "pair_groups = 3 needs kc = 16 (or kc = 0, auto)");
        // the keys are downloaded once per per-sketch pass: a later layout (next row block) needs no
        // device round trip and so does not wait for the work still queued on the stream
        const auto t_h0 = std::chrono::steady_clock::now();
        if (!c->hk32_valid && !reuse_host_layout) {
            HIPCHK(c, hipEventSynchronize(c->ev_keys));
            c->hk32_valid = true;
        }
        const auto t_h1 = std::chrono::steady_clock::now();
        c->host_keys_wait_us = std::chrono::duration<double, std::micro>(t_h1 - t_h0).count();
        const uint32_t *k32 = c->hk32;
        for (uint64_t i = c->card_from; i < n && !reuse_host_layout; ++i)  // (the sketches the per-sketch pass covered)
            if (plan::key_bad(k32[i]))
                return fail(c, DSH_EINVAL, "sketch %llu holds a register value above %d (= 64 - p + 1): not an HLL of precision %d (corrupt or foreign .hll?)",
                            (unsigned long long)i, 64 - c->p + 1, c->p);
        c->planes_valid = false;  // (the cached layout is overwritten from here on)
        plan::Layout &L = c->lay;
        if (!reuse_host_layout) {
            const plan::SketchWords words{k32, c->hg32, c->hv32, c->pass_sparse_cap};
            const plan::LayoutQuery query{want_sorted, want_rb, want_re, &parts, rowsorted ? std::max<uint32_t>(nparts, 1) : 0,
                                          extra->empty() ? nullptr : extra};
            plan::build_layout(n, words, query, L);
        }
        ++c->lay_serial;
        c->lay_built = true;
        c->cum_bytes = c->p <= 15 ? 2 : 4;
        const uint64_t m = 1ull << c->p;
        c->W = (uint32_t)std::max<uint64_t>(1, m / 32);
        // auto: three items per workgroup (and with them 16-row stages) wherever the lockstep kernel runs, unless the
        // caller asks for 32-row stages (profiles/r7g: -9 % of the step at C3, -3 % at 100 000 x p = 10, -11 % at p = 16)
        c->pair_groups = c->pair_groups_opt ? c->pair_groups_opt : (c->kc_opt == 32 ? 2 : 3);
        c->kc = c->pair_groups == 3 ? 16 : c->kc_opt ? c->kc_opt : (c->W >= 32 ? 32 : 16);
        if (want_sorted && !reuse_host_layout) {
            // perm, then (whole collection only) its inverse for the un-permute of the shard path
            const uint64_t nperm = L.perm.size();
            HIPCHK(c, c->perm.ensure(std::max<uint64_t>(nperm, 1) * sizeof(uint32_t)));
            if (nperm) {
                // one staging block (the previous layout's upload from it has run): perm, then where the rows of a
                // row-sorted rank's buffer start
                const size_t pb_ = (nperm * sizeof(uint32_t) + 15) & ~(size_t)15;
                const size_t rb_ = L.rowsorted ? L.rowoff.size() * sizeof(uint64_t) : 0;
                HIPCHK(c, c->st_perm.room(pb_ + rb_));
                uint8_t *h = (uint8_t *)c->st_perm.ptr();
                std::memcpy(h, L.perm.data(), nperm * sizeof(uint32_t));
                HIPCHK(c, launch_upload(c->stream, c->perm.ptr, h, nperm * sizeof(uint32_t)));
                if (L.rowsorted) {
                    HIPCHK(c, c->rowoff.ensure(rb_));
                    std::memcpy(h + pb_, L.rowoff.data(), rb_);
                    HIPCHK(c, launch_upload(c->stream, c->rowoff.ptr, h + pb_, rb_));
                }
                HIPCHK(c, c->st_perm.sent(c->stream));
            }
        }
        const uint32_t NT = L.Npad / kTile;
        // position index of every column block (the list joins of k_finalize): 79 workgroups at C3 -- built on a
        // second stream next to the bit-plane transform, which fills the chip on its own; both only need the
        // per-sketch pass and the permutation, the tile kernels wait for both
        c->nbuckets = (uint32_t)std::min<uint64_t>(2 * m, kMaxBuckets);  // (position group, upper | lower tail)
        c->ent_stride = std::max<uint32_t>(1, kTile * (uint32_t)(c->emax + c->elow));
        c->rl_stride = std::max<uint32_t>(1, (uint32_t)(c->emax + c->elow));
        const size_t nbk = std::max<size_t>(NT, 1);
        HIPCHK(c, c->cidx_rec.ensure(nbk * c->nbuckets * (size_t)(colindex_inline(c->p, c->rl_stride) + 1) * sizeof(uint32_t)));
        HIPCHK(c, c->cidx_ent.ensure(nbk * c->ent_stride * sizeof(uint32_t)));
        HIPCHK(c, c->colS_n.ensure(nbk * kTile * sizeof(uint32_t)));
        HIPCHK(c, c->colS_key.ensure(nbk * kTile * sizeof(uint32_t)));
        HIPCHK(c, c->colS_card.ensure(nbk * kTile * sizeof(double)));
        HIPCHK(c, c->colS_th.ensure(nbk * kTile * 64));
        HIPCHK(c, c->colS_rl.ensure(nbk * kTile * (size_t)c->rl_stride * sizeof(uint32_t)));
        c->host_layout_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_h1).count();
        HIPCHK(c, hipEventRecord(c->ev_aux_fork, c->stream));
        HIPCHK(c, hipStreamWaitEvent(c->aux_stream, c->ev_aux_fork, 0));
        {
            ColIndexLaunch ci;
            ci.exc = c->exc.ptr;
            ci.excv = (const uint8_t *)c->excv.ptr;
            ci.exc_n = (const uint32_t *)c->exc_n.ptr;
            ci.keys = (const uint32_t *)c->keys.ptr;
            ci.card = (const double *)c->card.ptr;
            ci.tailhist = (const uint8_t *)c->tailhist.ptr;
            ci.perm = want_sorted ? (const uint32_t *)c->perm.ptr : nullptr;
            ci.ncols = L.ncols;
            ci.p = c->p;
            ci.nblocks = NT;
            ci.nbuckets = c->nbuckets;
            ci.ent_stride = c->ent_stride;
            ci.E = c->rl_stride;
            ci.rec = (uint32_t *)c->cidx_rec.ptr;
            ci.ent = (uint32_t *)c->cidx_ent.ptr;
            ci.nS = (uint32_t *)c->colS_n.ptr;
            ci.keyS = (uint32_t *)c->colS_key.ptr;
            ci.cardS = (double *)c->colS_card.ptr;
            ci.thS = (uint8_t *)c->colS_th.ptr;
            ci.rl = (uint32_t *)c->colS_rl.ptr;
            HIPCHK(c, launch_build_colindex(c->aux_stream, ci));
        }
        HIPCHK(c, hipEventRecord(c->ev_aux_join, c->aux_stream));
        const uint64_t K = (uint64_t)L.P * c->W;
        c->Kpad = (uint32_t)((K + c->kc - 1) / c->kc * c->kc);
        if (c->Kpad) {
            const size_t bytes = (size_t)c->Kpad * L.Npad * sizeof(uint32_t);
            HIPCHK(c, c->planes.ensure(bytes));
            if (c->Kpad > K)
                HIPCHK(c, hipMemsetAsync((uint32_t *)c->planes.ptr + K * L.Npad, 0,
                                         (size_t)(c->Kpad - K) * L.Npad * sizeof(uint32_t),
                                         c->stream));
            HIPCHK(c, launch_transform(c->stream, c->regs, L.ncols, c->p, L.pbase, L.P, c->W, L.Npad,
                                       (uint32_t *)c->planes.ptr,
                                       want_sorted ? (const uint32_t *)c->perm.ptr : nullptr));
        }
        c->aux_join_pending = true;  // only k_finalize reads the index: the tile kernel starts without waiting for it
        c->lay_gen = c->pass_gen;
        c->planes_valid = true;
    }
    timer.stop(c->prep_ms, /*add=*/true);
    return DSH_OK;
}

// ---- run_pairs(): its steps, in the order they run ----
namespace {

// the layout a job runs on
struct JobLayout {
    int want_sorted = 0;
    uint64_t lrb = 0, lre = 0;  // the rows a key-ordered layout is made for
    bool with_parts = false;    // the job's parts become final one by one (an event or a flag per part)
    bool with_extra = false;    // further row segments behind the range (row sets, plan.h)
};

// what the steps of one call share
struct PairRun {
    plan::Tuning tu;
    std::vector<uint64_t> item_off;  // first item of every band in the call's item list (+ the end)
    plan::U4 *pinT = nullptr, *pinF = nullptr, *pinI = nullptr;  // page-locked staging: [tile kernel's list | k_finalize's list | items]
    bool signal = false;      // the parts announce themselves from inside k_finalize (else: an event per part)
    bool sig_upload = false;  // the signal block still has to travel (it goes with the first band's lists)
    FinalizeLaunch fin{};     // the call-invariant arguments of k_finalize; the band and the segment fill in theirs
    hipEvent_t e_call0 = nullptr;                             // (profiling, with parts) the call's start
    std::vector<std::pair<size_t, hipEvent_t>> ev_part_t;     // (profiling) part -> a timing event behind its last segment
    std::vector<std::pair<hipEvent_t, hipEvent_t>> evp, evf;  // (profiling) per band: around the tile kernel and the counting kernel, around k_finalize
    double build_in_pair_ms = 0;  // (profiling) k_sparse_build, which runs between the first band's two kernels and counts into prep_ms
};

// Triangle rows [rb,re): the plane matrix is laid out for exactly that range (wanted rows first, both
// parts key-ordered), so every tile is homogeneous and the result lands at its final packed position --
// whatever the range (a full triangle, one rank's rows, a row block of the CLI).  Tiny ranges and
// rectangles keep the identity layout, which stays cached across calls; a call with parts (an event per part:
// the pipelined exchange) always gets the key-ordered layout of its range, however short, so that its parts
// are the ones dsh_range_parts reports to the other ranks.
JobLayout choose_layout(const dsh_ctx *c, const PairJob &job)
{
    JobLayout jl;
    const uint64_t jre = std::min<uint64_t>(job.row_end, c->n);
    const bool full_tri = !job.rect && job.row_begin == 0 && jre >= c->n;
    jl.with_parts = job.nparts > 0 && !job.rect && !job.sorted_rows;
    jl.lre = c->n;
    if (job.sorted_rows) jl.want_sorted = 1;
    else if (!job.rect && jre > job.row_begin &&
             (jl.with_parts || (c->sort_mode != 0 && (full_tri || jre - job.row_begin >= (uint64_t)c->range_sort_min_rows)))) {
        jl.want_sorted = 1;
        jl.lrb = job.row_begin;
        jl.lre = jre;
    }
    // extra segments (row sets, plan.h): only with a key-ordered layout of the range and parts (the exchange)
    jl.with_extra = jl.want_sorted && jl.with_parts && !job.extra.empty() && jl.lre > jl.lrb;
    return jl;
}

// sparse outer planes (kernels_sparseplane.hip): the stride of a list row, and what a slab (table, lists, lengths) takes of
// the kSparseSlabBudget a call's slabs may fill (C3: 237 slabs of 576 KiB)
constexpr uint64_t kSparseSlabBudget = 2ull << 30;
uint32_t sparse_list_stride(const dsh_ctx *c)
{
    return std::max<uint32_t>(8, (std::min<uint32_t>((uint32_t)c->sparse_cap, plan::kSparseCapMax) + 7) / 8 * 8);
}
// the items a workgroup of the LDS placement takes one behind the other (option sparse_run; 0: the measured default)
uint32_t sparse_run_of(const dsh_ctx *c) { return c->sparse_run > 0 ? (uint32_t)c->sparse_run : plan::kSparseRunDefault; }
uint64_t sparse_slab_bytes(const dsh_ctx *c)
{
    return ((uint64_t)16 << c->p) + (uint64_t)kTile * sparse_list_stride(c) * sizeof(uint16_t) + kTile * sizeof(uint32_t);
}

plan::Tuning tuning_of(const dsh_ctx *c)
{
    plan::Tuning tu;
    tu.W = c->W;
    tu.kc = c->kc;
    tu.cum_bytes = c->cum_bytes;
    tu.cum_budget = c->cum_budget;
    tu.nsplit = c->nsplit;
    tu.lockstep = use_lockstep(c);
    tu.round_items = 256u * (uint32_t)c->pair_groups;  // a workgroup per CU, pair_groups items each
    tu.small_round_items = c->pair_groups_opt == 0 && c->pair_groups == 3 ? 512u : 0u;  // auto: a band may keep two where that costs less (plan.h)
    tu.part_band_tiles = (uint32_t)c->part_band_tiles;
    tu.overflow_frag_max_permille = (uint32_t)c->overflow_frag_permille;
    tu.tail_bands = (uint32_t)c->tail_bands;
    tu.p = c->p;
    tu.sparse_planes = c->sparse_planes;
    tu.sparse_cap = (uint32_t)c->sparse_cap;
    tu.sparse_sided = c->sparse_sided;
    tu.sparse_max_slabs = (uint32_t)std::min<uint64_t>(1u << 16, kSparseSlabBudget / sparse_slab_bytes(c));
    return tu;
}

// room for the call's lists on the device and in page-locked staging, and for a band's C(v)
int reserve_lists(dsh_ctx *c, PairRun &r)
{
    plan::PairPlan &pp = c->pp;
    const std::vector<plan::U4> &T = pp.T;
    r.item_off.assign(pp.bands.size() + 1, 0);
    for (size_t bi = 0; bi < pp.bands.size(); ++bi) r.item_off[bi + 1] = r.item_off[bi] + plan::band_item_count(r.tu, pp, bi);
    const uint64_t nitems_total = r.item_off.back();
    pp.items.reserve(nitems_total);
    // tile and item lists travel through page-locked staging, so nothing in the band loop needs the host to wait
    // (the previous call's upload is long done unless calls are issued back to back)
    static_assert(sizeof(plan::U4) == sizeof(uint4), "plan::U4 must have the layout of uint4");
    HIPCHK(c, c->st_lists.room((2 * T.size() + std::max<uint64_t>(nitems_total, 1)) * sizeof(uint4)));
    r.pinT = (plan::U4 *)c->st_lists.ptr(), r.pinF = r.pinT + T.size(), r.pinI = r.pinF + T.size();
    HIPCHK(c, c->tiles.ensure(2 * T.size() * sizeof(uint4)));  // [tile kernel's list | k_finalize's list]
    HIPCHK(c, c->items.ensure(std::max<uint64_t>(nitems_total, 1) * sizeof(uint4)));
    HIPCHK(c, c->cum.ensure(std::max<uint64_t>(pp.per_tile_bytes * pp.max_band, 256)));
    return DSH_OK;
}

// a signalling call's generation, and its signal block staged for the upload with the first band's lists
int stage_signal_block(dsh_ctx *c, PairRun &r)
{
    ++c->sig_gen;
    if (c->sig_gen == 0) c->sig_gen = 1;
    // the parts' tile totals (host -> device through page-locked staging), their counters cleared
    HIPCHK(c, c->st_sig.room((2 * kSigMaxParts + 2) * sizeof(uint32_t)));
    // the words kSigPartCnt .. kSigStamp of the block lie one behind the other: the parts' counters (zero), their totals,
    // the call's generation, the stamp switch -- uploaded with the first band's lists, in one launch (the tile counters
    // clear themselves: k_finalize_signal)
    static_assert(kSigPartTotal == kSigPartCnt + kSigMaxParts && kSigGen == kSigPartTotal + kSigMaxParts && kSigStamp == kSigGen + 1, "signal block layout");
    uint32_t *blk = (uint32_t *)c->st_sig.ptr(), *tot = blk + kSigMaxParts;
    for (uint32_t qd = 0; qd < kSigMaxParts; ++qd) blk[qd] = 0u;
    for (uint32_t qd = 0; qd < kSigMaxParts; ++qd) tot[qd] = qd < c->pp.part_tiles.size() ? c->pp.part_tiles[qd] : 0u;
    tot[kSigMaxParts] = c->sig_gen;                   // kSigGen
    tot[kSigMaxParts + 1] = c->profiling ? 1u : 0u;   // kSigStamp
    r.sig_upload = true;
    return DSH_OK;
}

// what every k_finalize launch of the call is given alike (the buffers are in place: nothing below moves them)
FinalizeLaunch finalize_invariants(const dsh_ctx *c, const PairJob &job, bool with_extra)
{
    const plan::Layout &L = c->lay;
    FinalizeLaunch f{};
    f.cum_bytes = c->cum_bytes;
    FinalizeArgs &a = f.a;
    a.cum = c->cum.ptr;  // the band's C(v); a tile's block is named by its descriptor
    a.perm = L.sorted ? (const uint32_t *)c->perm.ptr : nullptr;
    a.rowoff = L.rowsorted ? (const uint64_t *)c->rowoff.ptr : nullptr;
    a.pbase = L.pbase;
    a.p = c->p;
    a.estim = job.estim;
    a.result_type = job.result_type;
    a.ksinv = job.ksinv_double ? 1. / (double)job.k : (double)(float)(1. / (double)job.k);
    a.nS = (const uint32_t *)c->colS_n.ptr;
    a.keyS = (const uint32_t *)c->colS_key.ptr;
    a.cardS = (const double *)c->colS_card.ptr;
    a.thS = (const uint8_t *)c->colS_th.ptr;
    a.rl = (const uint32_t *)c->colS_rl.ptr;
    a.E = c->rl_stride;
    a.cidx_rec = (const uint32_t *)c->cidx_rec.ptr;
    a.cidx_ent = (const uint32_t *)c->cidx_ent.ptr;
    a.nbuckets = c->nbuckets;
    a.ent_stride = c->ent_stride;
    a.n = c->n;
    a.ncols = L.ncols;
    a.rect = job.rect;
    a.sorted_out = job.sorted_rows;
    a.square = job.square;
    a.knn = job.knn;
    a.out2 = job.d_out2;
    a.knn_ld = job.knn_ld;
    a.knn_rows = job.knn_rows;
    a.stop = c->finalize_stop;
    a.phase_cyc = c->finalize_timing ? (unsigned long long *)c->phase_cyc.ptr : nullptr;
    a.row_begin = job.row_begin;
    // (with extra segments every pair of a launched tile is this rank's: the runs of the layout lie in row order and
    // whole 128-column blocks are wanted or not, plan.h)
    a.row_end = with_extra ? c->n : job.row_end;
    a.col_begin = job.col_begin;
    a.col_end = job.col_end;
    a.base_index = job.base_index;
    a.out = job.d_out;
    return f;
}

// this band's items and list entries: planned, staged, uploaded (the uploads read the staging when they run: it is
// not touched again before st_lists' event of this call has passed)
int upload_band(dsh_ctx *c, PairRun &r, size_t bi)
{
    plan::PairPlan &pp = c->pp;
    const auto &bd = pp.bands[bi];
    const uint32_t nt = (uint32_t)(bd.second - bd.first);
    const size_t nT = pp.T.size();
    const auto t_b0 = std::chrono::steady_clock::now();
    plan::build_band_items(r.tu, pp, bi);
    if (pp.band_items[bi].first != r.item_off[bi] || pp.band_items[bi].second != r.item_off[bi + 1])
        return fail(c, DSH_EIO, "internal: band %zu has %zu items, %llu were planned for", bi,
                    pp.band_items[bi].second - pp.band_items[bi].first, (unsigned long long)(r.item_off[bi + 1] - r.item_off[bi]));
    plan::emit_band_lists(c->lay, pp, bi, r.pinT, r.pinF);
    const uint32_t ni = (uint32_t)(r.item_off[bi + 1] - r.item_off[bi]);
    if (ni) std::memcpy(r.pinI + r.item_off[bi], pp.items.data() + r.item_off[bi], (size_t)ni * sizeof(uint4));
    c->host_lists_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_b0).count();
    UploadSegs up;
    uint32_t nseg = 0;
    if (r.sig_upload) up.add(nseg, (uint32_t *)c->sig.ptr + kSigPartCnt, c->st_sig.ptr(), (2 * kSigMaxParts + 2) * sizeof(uint32_t));
    up.add(nseg, (uint4 *)c->tiles.ptr + bd.first, r.pinT + bd.first, (size_t)nt * sizeof(uint4));
    up.add(nseg, (uint4 *)c->tiles.ptr + nT + bd.first, r.pinF + bd.first, (size_t)nt * sizeof(uint4));
    up.add(nseg, (uint4 *)c->items.ptr + r.item_off[bi], r.pinI + r.item_off[bi], (size_t)ni * sizeof(uint4));
    HIPCHK(c, launch_upload_segs(c->stream, up, nseg));
    if (r.sig_upload) {
        HIPCHK(c, c->st_sig.sent(c->stream));
        r.sig_upload = false;
    }
    HIPCHK(c, c->st_lists.sent(c->stream));
    return DSH_OK;
}

// The slabs of the call's sparse items (built unless the buffers hold exactly them, of this layout) and the items
// themselves on the device, once per call behind plan::emit_sparse_items.  Behind prepare() on the same stream: the
// bit-plane matrix the slabs are made from is there.
int prepare_sparse(dsh_ctx *c)
{
    const plan::PairPlan &pp = c->pp;
    const plan::Layout &L = c->lay;
    const size_t ns = pp.slabs.size(), ni = pp.sp_items.size();
    const uint32_t cap = sparse_list_stride(c);
    const uint64_t m = 1ull << c->p;
    static_assert(sizeof(plan::U2) == sizeof(uint2), "plan::U2 must have the layout of uint2");
    HIPCHK(c, c->sp_items.ensure(ni * sizeof(uint4)));
    HIPCHK(c, c->sp_slabs.ensure(ns * sizeof(uint2)));
    const size_t ib = ni * sizeof(uint4), sb = ns * sizeof(uint2);
    HIPCHK(c, c->st_sparse.room(ib + sb));
    uint8_t *h = (uint8_t *)c->st_sparse.ptr();
    std::memcpy(h, pp.sp_items.data(), ib);
    std::memcpy(h + ib, pp.slabs.data(), sb);
    HIPCHK(c, launch_upload(c->stream, c->sp_items.ptr, h, ib));
    const bool have = c->sp_serial == c->lay_serial && c->sp_cap_have == (cap | (uint32_t)sparse_wordmajor(c) << 31) && c->sp_have.size() == ns &&
                      std::memcmp(c->sp_have.data(), pp.slabs.data(), sb) == 0;
    if (!have) {
        DeviceTimer timer(c, c->stream);
        c->sp_have.clear();
        HIPCHK(c, launch_upload(c->stream, c->sp_slabs.ptr, h + ib, sb));
        HIPCHK(c, c->sp_tab.ensure(ns * m * 16));
        HIPCHK(c, c->sp_lists.ensure(ns * kTile * (size_t)cap * sizeof(uint16_t)));
        HIPCHK(c, c->sp_len.ensure(ns * kTile * sizeof(uint32_t)));
        HIPCHK(c, launch_sparse_build(c->stream, (const uint32_t *)c->planes.ptr, L.Npad, c->W, L.ncols, (const uint2 *)c->sp_slabs.ptr,
                                      (uint32_t)ns, cap, sparse_wordmajor(c), (uint32_t *)c->sp_tab.ptr, (uint16_t *)c->sp_lists.ptr, (uint32_t *)c->sp_len.ptr));
        c->sp_have = pp.slabs;
        c->sp_serial = c->lay_serial;
        c->sp_cap_have = cap | (uint32_t)sparse_wordmajor(c) << 31;
        timer.stop(c->prep_ms, /*add=*/true);
    }
    HIPCHK(c, c->st_sparse.sent(c->stream));
    return DSH_OK;
}

// the band's sparse items, behind its tile kernel: both fill the band's C(v), k_finalize needs both
int launch_sparse_items(dsh_ctx *c, size_t bi, uint64_t nslots)
{
    const plan::PairPlan &pp = c->pp;
    if (bi >= pp.band_sp_items.size()) return DSH_OK;
    const auto &rg = pp.band_sp_items[bi];
    if (rg.first == rg.second) return DSH_OK;
    hipEvent_t a = c->profiling ? next_event(c) : nullptr, b = c->profiling ? next_event(c) : nullptr;
    if (a && b) (void)hipEventRecord(a, c->stream);
    if (sparse_wordmajor(c)) c->sparse_run_used = sparse_run_of(c);
    HIPCHK(c, launch_sparse_count(c->stream, c->cum_bytes, (const uint4 *)c->sp_items.ptr + rg.first, (uint32_t)(rg.second - rg.first),
                                  sparse_run_of(c), sparse_wordmajor(c), sparse_words_of(c), (const uint32_t *)c->sp_tab.ptr, (const uint16_t *)c->sp_lists.ptr, (const uint32_t *)c->sp_len.ptr,
                                  sparse_list_stride(c), 1u << c->p, c->cum.ptr, nslots));
    if (a && b) {
        (void)hipEventRecord(b, c->stream);
        c->ev_sparse.emplace_back(a, b);
    }
    return DSH_OK;
}

int launch_tile_kernel(dsh_ctx *c, const PairRun &r, size_t bi, uint64_t nslots)
{
    const plan::Layout &L = c->lay;
    const plan::PairPlan &pp = c->pp;
    const uint4 *dt = (const uint4 *)c->tiles.ptr + pp.bands[bi].first;
    const uint4 *di = (const uint4 *)c->items.ptr + r.item_off[bi];
    const uint32_t ni = (uint32_t)(r.item_off[bi + 1] - r.item_off[bi]);
    if (c->pair_mfma)
        HIPCHK(c, launch_pair_counts_mfma(c->stream, c->kc, c->cum_bytes, (const uint32_t *)c->planes.ptr,
                                          L.Npad, c->Kpad, c->W, L.P, dt, di, ni, c->cum.ptr, nslots));
    else if (use_lockstep(c))
        HIPCHK(c, launch_pair_counts_lockstep(c->stream, c->kc, (int)(pp.band_round[bi] / 256), c->cum_bytes, (const uint32_t *)c->planes.ptr,
                                              L.Npad, c->Kpad, c->W, L.P, dt, di, ni, bi < pp.band_frags.size() ? pp.band_frags[bi] : 0u,
                                              c->cum.ptr, nslots));
    else
        HIPCHK(c, launch_pair_counts(c->stream, c->kc, c->cum_bytes, (const uint32_t *)c->planes.ptr,
                                     L.Npad, c->Kpad, c->W, L.P, dt, di, ni, c->cum.ptr, nslots));
    return DSH_OK;
}

// k_finalize over one band, and the marks of the parts it completes
int finalize_band(dsh_ctx *c, PairRun &r, size_t bi)
{
    const plan::PairPlan &pp = c->pp;
    const auto &bd = pp.bands[bi];
    // signal mode: ONE launch over the band's tiles; the parts announce themselves (k_finalize_signal)
    std::vector<plan::Seg> one_seg;
    if (r.signal) {
        plan::Seg all{bd.first, bd.second, -1, 1};
        for (const plan::Seg &sg : pp.segs[bi]) all.hist_bins = std::max(all.hist_bins, sg.hist_bins);
        one_seg.push_back(all);
    }
    // (without flags -- finalize_signal = 0, or a device without stream wait-value -- one launch and one event per part)
    for (const plan::Seg &sg : r.signal ? one_seg : pp.segs[bi]) {
        hipStream_t fst = c->stream;
        FinalizeLaunch &f = r.fin;
        f.a.hist_bins = sg.hist_bins;
        f.a.tiles = (const uint4 *)c->tiles.ptr + pp.T.size() + sg.b;
        f.nslots = (uint64_t)(sg.e - sg.b) * kTile * kTile;
        f.a.sig = r.signal ? (uint32_t *)c->sig.ptr : nullptr;
        if (c->aux_join_pending) {  // (the position index is built on the second stream)
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_aux_join, 0));
            c->aux_join_pending = false;
        }
        HIPCHK(c, launch_finalize(fst, f));
        if (sg.part >= 0) {  // this segment completes a part: its span of the matrix is final
            const size_t qp = (size_t)sg.part;
            while (c->ev_part.size() <= qp) HIPCHK(c, add_event(c->ev_part));
            HIPCHK(c, hipEventRecord(c->ev_part[qp], fst));
            c->parts_done = (uint32_t)qp + 1;
            if (r.e_call0) {
                hipEvent_t te = next_event(c);
                if (te) {
                    (void)hipEventRecord(te, fst);
                    r.ev_part_t.emplace_back(qp, te);
                }
            }
        }
    }
    return DSH_OK;
}

// (profiling) waits for the call and reads its timing events back
int read_profile(dsh_ctx *c, const PairRun &r)
{
    const plan::Layout &L = c->lay;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (auto &e : r.evp) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e.first, e.second);
        c->pair_ms += ms;
        if (c->Kpad) c->pair_launches++;
    }
    c->pair_ms -= r.build_in_pair_ms;  // (the first band's interval holds k_sparse_build: that is prep_ms')
    for (auto &e : r.evf) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e.first, e.second);
        c->fin_ms += ms;
    }
    c->sparse_ms = 0;
    for (auto &e : c->ev_sparse) {  // (inside the tile kernels' intervals above: pair_ms holds them too)
        float ms = 0;
        (void)hipEventElapsedTime(&ms, e.first, e.second);
        c->sparse_ms += ms;
    }
    c->ev_sparse.clear();
    // when every part of the call was final (from the start of the call, prepare included) and how many floats of the
    // rank's buffer it holds: what a model of the pipelined exchange needs (dsh_last_part_info)
    auto fill_part_floats = [&] {  // how many floats of the rank's buffer every part holds
        for (size_t i = 0; i < c->part_floats.size(); ++i) {
            if (L.rowsorted && i + 1 < L.part_w.size()) c->part_floats[i] = L.rowoff_w[L.part_w[i + 1]] - L.rowoff_w[L.part_w[i]];
            else if (!L.rowsorted && L.extra.empty() && i + 1 < L.parts.size()) c->part_floats[i] = plan::tri_span(c->n, L.parts[i], L.parts[i + 1]);
            else if (!L.rowsorted) c->part_floats[i] = plan::rowset_span(c->n, L.rb, L.re, L.extra);
        }
    };
    if (r.signal && r.e_call0 && c->wall_clock_khz > 0) {
        std::vector<unsigned long long> st(kSigMaxParts + 1);
        HIPCHK(c, hipMemcpy(st.data(), (uint32_t *)c->sig.ptr + kSigPartTime, kSigMaxParts * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(&st[kSigMaxParts], (uint32_t *)c->sig.ptr + kSigT0, sizeof(unsigned long long), hipMemcpyDeviceToHost));
        c->part_ready_ms.assign(c->parts_done, 0.0);
        c->part_floats.assign(c->parts_done, 0);
        for (size_t i = 0; i < c->part_ready_ms.size(); ++i)
            c->part_ready_ms[i] = (double)(long long)(st[i] - st[kSigMaxParts]) / (double)c->wall_clock_khz;
        fill_part_floats();
    } else if (r.e_call0 && !r.ev_part_t.empty()) {
        c->part_ready_ms.assign(c->parts_done, 0.0);
        c->part_floats.assign(c->parts_done, 0);
        for (auto &pe : r.ev_part_t) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, r.e_call0, pe.second);
            if (pe.first < c->part_ready_ms.size()) c->part_ready_ms[pe.first] = ms;
        }
        fill_part_floats();
    }
    return DSH_OK;
}

}  // namespace

int run_pairs(dsh_ctx *c, const PairJob &job)
{
    PairRun r;
    const JobLayout jl = choose_layout(c, job);
    c->parts_done = 0;
    c->part_ready_ms.clear();
    c->part_floats.clear();
    if (jl.with_parts) {  // the signal block of the parts (kernels.h kSig*; used when the call turns out to signal, below)
        HIPCHK(c, c->sig.ensure((size_t)kSigWords * sizeof(uint32_t)));
        if (c->sig_gen == 0) {  // (first use: the flags must not hold garbage that passes for a generation)
            HIPCHK(c, hipMemsetAsync(c->sig.ptr, 0, (size_t)kSigWords * sizeof(uint32_t), c->stream));  // (and the tile counters, which clear themselves from then on)
            c->sig_gen = 1;
        }
    }
    if (c->profiling && jl.with_parts) {
        r.e_call0 = next_event(c);
        if (r.e_call0) (void)hipEventRecord(r.e_call0, c->stream);
        // the call's start on the device's wall clock: signalled parts stamp their completion on the same
        HIPCHK(c, launch_wall_stamp(c->stream, reinterpret_cast<unsigned long long *>((uint32_t *)c->sig.ptr + kSigT0)));
    }
    if (!job.extra.empty() && !jl.with_extra) return fail(c, DSH_EINVAL, "internal: extra row segments need a key-ordered range with parts");
    int rc = prepare(c, job.estim, jl.want_sorted, false, jl.lrb, jl.lre, jl.with_parts ? job.nparts : 1, jl.with_parts && job.rowsorted,
                     jl.with_extra ? &job.extra : nullptr);
    if (rc) return rc;
    if (job.result_type < 0 || job.result_type > 8)
        return fail(c, DSH_EINVAL, "unsupported result_type %d", job.result_type);
    if (job.k < 1) return fail(c, DSH_EINVAL, "bad k %d", job.k);
    if (sparse_words_of(c) == 2 && c->p > 14) return fail(c, DSH_EINVAL, "sparse_words = 2 needs p <= 14: a word pair of the table at p = %d does not fit a CU's LDS", c->p);
    const auto t_l0 = std::chrono::steady_clock::now();
    plan::PairPlan &pp = c->pp;
    plan::PairQuery q;
    q.rect = job.rect;
    q.sorted_rows = job.sorted_rows;
    q.want_parts = jl.with_parts;
    q.row_begin = job.row_begin;
    q.row_end = job.row_end;
    q.col_begin = job.col_begin;
    q.col_end = job.col_end;
    r.tu = tuning_of(c);
    // Tiles, bands and segments of the whole job first; the work items and the two device lists are made, uploaded and
    // launched BAND BY BAND: the host plans band b + 1 while the GPU runs band b (at 100 000 x p=10 the plan of 306 000
    // tiles took the host 8 ms that nothing hid, round 4 / profiles/r4y).  Of the sparse routes build_tiles only decides
    // which planes leave the tile kernel; their items are emitted in the band loop below, behind the first tile kernel.
    if (!plan::build_tiles(c->lay, q, r.tu, pp)) {
        pp.T.clear();
        return DSH_OK;
    }
    c->last_bands = pp.bands.size();
    if ((rc = reserve_lists(c, r))) return rc;
    c->host_lists_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_l0).count();  // (until the first band can be planned)

    // Part signalling (kernels.h, k_finalize_signal): with parts, ONE k_finalize launch per band; the parts' flags are
    // written from inside it and the copy stream waits for them with hipStreamWaitValue32 (exchange.hip).  Not with the
    // stamped / general instances (profiling aids, rectangles) and not where the device lacks stream wait-value.
    if (jl.with_parts && pp.nparts >= 1 && pp.nparts <= kSigMaxParts && !c->finalize_timing && !c->finalize_stop && c->finalize_signal != 0) {
        r.signal = device_can_wait_value(c);
        if (!r.signal && c->finalize_signal == 1) return fail(c, DSH_ENODEV, "option finalize_signal = 1, but the device does not support hipStreamWaitValue32");
    }
    c->parts_signalled = r.signal;
    if (r.signal && (rc = stage_signal_block(c, r))) return rc;
    if (c->finalize_timing) {
        HIPCHK(c, c->phase_cyc.ensure(16 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemsetAsync(c->phase_cyc.ptr, 0, 16 * sizeof(unsigned long long), c->stream));
    }
    r.fin = finalize_invariants(c, job, jl.with_extra);
    c->ev_sparse.clear();
    c->sparse_run_used = 0;
    c->host_sparse_us = 0;
    for (size_t bi = 0; bi < pp.bands.size(); ++bi) {
        const uint64_t nslots = (uint64_t)(pp.bands[bi].second - pp.bands[bi].first) * kTile * kTile;
        if ((rc = upload_band(c, r, bi))) return rc;
        hipEvent_t a = nullptr, b = nullptr, d = nullptr;
        if (c->profiling) {
            a = next_event(c);
            b = next_event(c);
            d = next_event(c);
            if (a) (void)hipEventRecord(a, c->stream);
        }
        if ((rc = launch_tile_kernel(c, r, bi, nslots))) return rc;
        if (bi == 0) {  // (the destination of an exchange may post its receives behind its first tile kernel, exchange.hip)
            HIPCHK(c, c->ev_first_tiles.ensure());
            HIPCHK(c, hipEventRecord(c->ev_first_tiles, c->stream));
        }
        // The sparse items of the whole call are emitted and ordered here, behind the first band's tile kernel: only the
        // counting kernel needs them, and the host's time for them (host_sparse_us) passes while that kernel runs.  The two
        // kernels write disjoint slots of the band's C(v); k_finalize below is behind both.
        if (bi == 0 && pp.sp_count) {
            const auto t_s0 = std::chrono::steady_clock::now();
            plan::emit_sparse_items(c->lay, pp);
            c->host_sparse_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_s0).count();
            const double prep0 = c->prep_ms;
            if ((rc = prepare_sparse(c))) return rc;
            r.build_in_pair_ms = c->prep_ms - prep0;
        }
        if ((rc = launch_sparse_items(c, bi, nslots))) return rc;
        if (b) (void)hipEventRecord(b, c->stream);
        r.fin.a.nslots = nslots;  // (the band's stride: the distance between two planes of its C(v))
        if ((rc = finalize_band(c, r, bi))) return rc;
        if (d) (void)hipEventRecord(d, c->stream);
        if (a && b && d) {
            r.evp.emplace_back(a, b);
            r.evf.emplace_back(b, d);
        }
    }
    if (r.signal) c->parts_done = pp.nparts;  // (every part's flag will be written by the launches above)
    // everything is enqueued; the blocking entry points synchronise, the *_async ones return here
    return c->profiling ? read_profile(c, r) : DSH_OK;
}

}  // namespace dsh
