// ctx.h -- the per-GPU context behind the opaque dsh_ctx of include/dashing_hip.h, the owners of what it holds on the
// device and in page-locked memory (DevBuf, PinBuf, Event, Stream, Staging: each releases itself, so `delete` of a
// context is its whole release list), and the internal entry points the translation units of libdashing_hip.so share:
//   abi.hip       context, resident sketches, cardinalities, compare entry points, tickets, shards, options
//   sketch.hip    the sketch waist: dsh_sketch_batch*, dsh_sketch_records*, dsh_sketch_fastx_batch_async
//   sketch_plan.h (header, no HIP types) the lists the host fills for the sketch kernels and the planners that cut them
//   engine.hip    prepare() (per-sketch pass, layout, bit-planes, position index) and run_pairs() (tile kernel + k_finalize)
//   knn.hip       dsh_knn
//   bands.h       (header) the band walk of the five consumers of dense bands: threshold, cluster, greedy, greedy_extend,
//                 group_stats -- band rule (plan.cpp), geometry, run_pairs into thr_vals, a callback per band
//   threshold.hip dsh_dist_threshold*, dsh_dist_rect_threshold (values that pass a threshold, as CSR)
//   pairs.hip     dsh_dist_pairs* (values of an explicit list of pairs, the direct form)
//   cluster.hip   dsh_cluster_* (connected components at a threshold, or of a caller's graph)
//   mst.hip       dsh_mst* (the minimum spanning tree of the pair values: the single-linkage dendrogram)
//   dbscan.hip    dsh_dbscan_*, dsh_degree_threshold* (density clusters at a threshold; the degrees of the threshold graph)
//   greedy.hip    dsh_greedy_threshold* (greedy representatives at a threshold, in slot order)
//   greedy_extend.hip  dsh_greedy_extend* (the same behind a labelling of the first slots; first or best representative)
//   group_stats.hip    dsh_group_stats* (per-group statistics and medoids of a labelling)
//   hist.hip      dsh_dist_histogram*, dsh_dist_rect_histogram (the distribution of the values over caller-given edges)
//   derive.hip    dsh_fold*, dsh_upload_sketches_folded*, dsh_union_groups* (new sketches out of resident ones)
//   curve.hip     dsh_union_curve*, dsh_curve_permutations (the growth of the union along orders of resident sketches)
//   curve_plan.h  (header, no HIP types) the cut of those orders into segments and batches
//   comm.hip      RCCL: the loader, dsh_comm_*, dsh_allgather_device, the guarded wait, the poster of a grouped round
//   exchange.hip  dsh_collect_*, dsh_exchange_*, dsh_dist_collect, the one-GPU diagnostics of the exchange
//   exchange_plan.h  (header, no HIP types) the modes of the ranks, the round schedule of dsh_exchange_collect_async
//   kernels_exchange.hip  row placement at the destination, the un-permute, the diagnostics' kernels
//   plan.cpp      the pure-host planner (layout, tiles, bands, parts, work items, row partitions, shard bounds)
// State that one of these modules uses alone is a named member struct of dsh_ctx (c->cc.parent, c->xch.comm); what the
// compare path shares with every module stays flat.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is dlopen'ed at dsh_comm_init (single-GPU users never load it)

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <string>
#include <vector>

#include "../../include/dashing_hip.h"
#include "kernels.h"
#include "plan.h"

// The owners below free in their destructors and are neither copied nor moved (a pool of them is a std::deque, which
// never relocates).  Scratch stays grow-only: nothing is freed before its owner goes, except by ensure() making room.
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

struct DevBuf : NoCopy {
    void *ptr = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        hipError_t e = hipMalloc(&ptr, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release()
    {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

// page-locked host memory: a hipMemcpyAsync from or to it is a true asynchronous DMA, so the call that enqueued it may
// return before the copy has run
struct PinBuf : NoCopy {
    void *ptr = nullptr;
    size_t cap = 0;
    ~PinBuf() { release(); }
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        release();
        const size_t want = bytes + bytes / 2;
        hipError_t e = hipHostMalloc(&ptr, want, hipHostMallocDefault);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release()
    {
        if (ptr) (void)hipHostFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

// one word of page-locked memory the device reads through a mapping (dsh_diag_spin_*)
struct MappedWord : NoCopy {
    uint32_t *ptr = nullptr;
    ~MappedWord() { if (ptr) (void)hipHostFree(ptr); }
    hipError_t ensure() { return ptr ? hipSuccess : hipHostMalloc((void **)&ptr, 64, hipHostMallocMapped); }
};

// an event made on first use: ensure() returns the creation's error (its caller's HIPCHK reports it)
struct Event : NoCopy {
    hipEvent_t ev = nullptr;
    ~Event() { if (ev) (void)hipEventDestroy(ev); }
    hipError_t ensure(unsigned flags = hipEventDisableTiming) { return ev ? hipSuccess : hipEventCreateWithFlags(&ev, flags); }
    operator hipEvent_t() const { return ev; }
};

// one more event at the end of a pool; a pool never holds an event that could not be made
inline hipError_t add_event(std::deque<Event> &pool, unsigned flags = hipEventDisableTiming)
{
    pool.emplace_back();
    const hipError_t e = pool.back().ensure(flags);
    if (e != hipSuccess) pool.pop_back();
    return e;
}

struct Stream : NoCopy {
    hipStream_t st = nullptr;
    ~Stream() { if (st) (void)hipStreamDestroy(st); }
    hipError_t create() { return st ? hipSuccess : hipStreamCreateWithFlags(&st, hipStreamNonBlocking); }
    // The copy-out stream gets the highest priority the device offers: on this runtime a device-to-host copy that has to
    // wait for an event of another stream runs as a small blit kernel, which would otherwise queue behind the millions
    // of workgroups of the compare kernels it is meant to overlap with (profiles/r3d).
    hipError_t create_copy()
    {
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) greatest = 0;
        if (const char *e = std::getenv("DSH_COPY_STREAM_PRIORITY")) greatest = std::atoi(e);
        return hipStreamCreateWithPriority(&st, hipStreamNonBlocking, greatest);
    }
    operator hipStream_t() const { return st; }
};

// Page-locked staging of an upload: filled by the host, read by a copy or an upload kernel when the stream gets there, so
// the call that filled it may return first.  The block may be rewritten -- and may MOVE, since growing frees the old
// block under a DMA that still reads it -- only once the previous upload has run: room() waits first and grows second.
struct Staging : NoCopy {
    PinBuf buf;
    Event sent_ev;
    bool in_flight = false;
    // the previous upload has run (for a caller whose size is only known later: room() waits anyway)
    hipError_t wait()
    {
        if (!in_flight) return hipSuccess;
        const hipError_t e = hipEventSynchronize(sent_ev);
        if (e == hipSuccess) in_flight = false;
        return e;
    }
    // room for `bytes` to write: waits for the previous upload if one is in flight
    hipError_t room(size_t bytes)
    {
        const hipError_t e = wait();
        return e == hipSuccess ? buf.ensure(bytes) : e;
    }
    // the upload has been enqueued on `st`
    hipError_t sent(hipStream_t st)
    {
        hipError_t e = sent_ev.ensure();
        if (e == hipSuccess) e = hipEventRecord(sent_ev, st);
        if (e == hipSuccess) in_flight = true;
        return e;
    }
    void *ptr() const { return buf.ptr; }
};

// DESTRUCTION ORDER: members go in reverse order of declaration, and `delete` of a context is what frees its buffers and
// events (abi.hip: release_ctx has made the device current, waited for every stream and released the communicator just
// before).  The streams are therefore declared FIRST, so that they go last, behind every buffer, staging block and event
// that was used on them; a new member goes below them.
struct dsh_ctx {
    int device = 0;
    Stream stream;
    // copy-out pipeline of dsh_dist_rows_async: results alternate between two device buffers; the copy of call b to the
    // host runs on its own stream while the kernels of call b+1 fill the other buffer
    Stream copy_stream;
    Stream aux_stream;    // prepare(): the column index is built next to the bit-plane transform
    Stream place_stream;  // destination of an exchange: received rows are put into place beside the next round's transfer
    Stream spin_stream;   // diagnostics (dsh_diag_spin_*): the waiting kernel's own
    std::string err;
    // resident sketch matrix
    DevBuf regs_own;
    const uint8_t *regs = nullptr;  // device
    uint64_t n = 0;
    int p = 0;
    bool have_sketches = false;
    // derived state
    bool planes_valid = false;
    int card_estim = -1;
    uint64_t card_from = 0;             // the per-sketch pass (cardinalities, lists, keys) covers the sketches [card_from, n)
    uint64_t pass_gen = 0, lay_gen = 0; // per-sketch passes so far; the one the layout's per-column data was built from
    DevBuf card, planes, cum, tiles, items, outbuf, exc, excv, exc_n, keys, perm, tailhist;
    Event ev_aux_fork, ev_aux_join;
    bool aux_join_pending = false;
    DevBuf outbuf2[2];
    Event ev_filled[2];                 // kernels of the call that filled outbuf2[b] done (recorded on stream)
    Event ev_drained[2];                // copy out of outbuf2[b] done (recorded on copy_stream)
    bool drained_pending[2] = {false, false};
    unsigned out_turn = 0;
    std::deque<Event> tickets;          // dsh_event_record ring: slot t % 64 holds {mark on the ctx stream, mark on the copy stream}
    uint64_t ticket_next = 0;
    Event ev_first_tiles;               // the tile kernel of the last call's first band has run
    bool pass_from_zero = false;        // the next per-sketch pass covers every sketch (the destination of an exchange)
    DevBuf hist;                        // [n][64] per-sketch register histograms (k_selfhist_card -> k_card_from_hist)
    Event ev_keys;                      // the keys have reached the host
    DevBuf cidx_rec, cidx_ent;          // position index of the column blocks of the current layout (k_build_colindex)
    uint32_t nbuckets = 0, ent_stride = 0;
    DevBuf colS_n, colS_key, colS_card, colS_th, colS_rl;  // per column of the layout, in layout order (k_finalize's inputs)
    uint32_t rl_stride = 0;             // entries of a compact list row (emax + elow)
    // column layout of the cached plane matrix (plan.h) and the plan of the last compare call
    dsh::plan::Layout lay;
    bool lay_built = false;             // `lay` holds a layout (whatever happened to the planes since)
    dsh::plan::PairPlan pp;
    std::deque<Event> ev_part;          // part q complete (recorded on the ctx stream by the last call with parts)
    uint32_t parts_done = 0;            // parts of the last dsh_dist_rows_parts_device_async call
    // part signalling (kernels.h kSig*): k_finalize announces the parts from inside ONE launch per band; the copy stream
    // waits for a part's flag with hipStreamWaitValue32 instead of an event between launches
    DevBuf sig;
    Staging st_sig;                     // the parts' tile totals on their way to the device
    uint32_t sig_gen = 0;               // generation of the last call with parts: the value its flags take
    bool parts_signalled = false;       // the last call with parts used flags (else events)
    int finalize_signal = -1;           // option: -1 auto (on where the device supports stream wait-value), 0 events, 1 flags
    int can_wait_value = -1;            // hipDeviceAttributeCanUseStreamWaitValue, queried once
    int wall_clock_khz = 0;
    PinBuf pin_keys;                    // host copy of the per-sketch keys (valid while the per-sketch pass is), page-locked:
    const uint32_t *hk32 = nullptr;     // the copy is a direct DMA and the host only waits for ev_keys
    const uint32_t *hg32 = nullptr;     // the per-sketch counts g0 | g1 << 16 behind the keys, same transfer (plan.h, build_layout)
    const uint32_t *hv32 = nullptr;     // and behind those the thresholds vU | vA << 8 of the sided route, computed at the cap ...
    uint32_t pass_sparse_cap = 0;       // ... sparse_cap had when the per-sketch pass ran (plan.h, Layout::thr_cap)
    bool hk32_valid = false;
    double host_layout_us = 0, host_lists_us = 0, host_keys_wait_us = 0;  // host time of the last call (dsh_get_info)
    double host_sparse_us = 0;  // ... and of its plan::emit_sparse_items, which runs behind the first band's tile kernel
    Staging st_perm;                    // lay.perm, then (row-sorted parts) lay.rowoff from the next 16-byte boundary on
    DevBuf rowoff;                      // (row-sorted parts) offset of the row at layout position s in the rank's buffer
    Staging st_lists;                   // tiles then items of the call in flight
    uint32_t W = 0, Kpad = 0;           // words per plane; plane rows padded to whole LDS stages
    int emax = 0, elow = 0, cum_bytes = 4;
    // options
    int kc = 16;      // k-rows per LDS stage in effect (set by prepare from kc_opt)
    int kc_opt = 0;   // 0 auto: 16 with three items per workgroup (the default); with two, 32 where a plane is at least that long (p >= 10)
    int pair_groups = 3;      // lockstep tile kernel: work items per workgroup of 256 x pair_groups threads in effect (set by prepare)
    int pair_groups_opt = 0;  // 0 auto (3, or 2 where kc = 32 is asked for; a band of <= 512 items keeps 2: plan.h) | 2 | 3 (3 needs
                              // kc = 16: auto kc becomes 16)
    int emax_opt = -1;  // cap of the listed upper tail; -1: auto_list_cap(p, true)
    int elow_opt = -1;  // cap of the listed lower tail; -1: auto_list_cap(p, false)
    int part_band_tiles = 2048;       // a part of at least this many tiles gets its own launch of the tile kernel (plan.cpp)
    int overflow_frag_permille = 500;  // overflow fragments of the tile kernel (plan.h, Tuning): 0 = never
    int sparse_planes = -1;  // sparse outer planes (plan.h, Tuning): -1 auto, 0 off, 1 | 2 forced
    int sparse_cap = (int)dsh::plan::kSparseCapDefault;  // the longest set a routed plane may have
    int sparse_sided = -1;   // the sided route (plan.h, Tuning::sparse_sided): -1 auto, 0 off, 1 forced
    int sparse_lds = 1;      // the table of the counting kernel staged in LDS where a word of it fits (p <= 15); 0: gathered
    int sparse_run = 0;      // items a workgroup of the LDS placement takes one behind the other (plan.h, sparse_table_fills); 0: kSparseRunDefault
    int sparse_words = 0;    // table words a workgroup of the LDS placement stages side by side: 1 | 2 (p <= 14); 0: 1, the measured choice
    uint32_t sparse_run_used = 0;  // the run of the last call's launches of the LDS placement; 0: it had none
    DevBuf sp_tab, sp_lists, sp_len, sp_slabs, sp_items;  // the slabs of the last call that routed planes (kernels_sparseplane.hip) and its items
    Staging st_sparse;               // slabs then sparse items on their way to the device
    std::vector<dsh::plan::U2> sp_have;  // the slabs sp_tab / sp_lists / sp_len hold ...
    uint64_t sp_serial = 0, lay_serial = 0;  // ... of which layout (lay_serial counts the layouts built)
    uint32_t sp_cap_have = 0;
    double sparse_ms = 0;            // (profiling) the counting kernel of the last call
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_sparse;  // (profiling) around its launches
    int tail_bands = 2;  // option xch_tail_bands: small jobs with parts have their tile kernel cut at whole rounds (plan.h, Tuning)
    std::vector<double> part_ready_ms;  // (profiling) when each part of the last call with parts was final, from the call's start
    std::vector<uint64_t> part_floats;  // and the floats of the rank's buffer it holds
    size_t last_bands = 0;            // tile-kernel launches groups (bands) of the last dist call
    uint64_t cum_budget = 8ull << 30;  // scratch for C(v) per pair slot: larger jobs run in bands (2 -> 8 GiB: -1.5 % at 100 000 x p=10)
    int sort_mode = -1;  // -1 auto (key-ordered columns for triangle calls of >= range_sort_min_rows rows), 0 never
    int range_sort_min_rows = 1024;  // smaller row ranges keep the cached identity layout (a rebuild costs more than it saves)
    DevBuf thr_vals;                  // a band's dense values (bands.h: every band consumer)
    uint64_t threshold_band_bytes = (uint64_t)1 << 30;  // a band (bands.h) holds at most this much float32
    uint64_t knn_square_budget = (uint64_t)96 << 30;  // all-vs-all kNN keeps an n x n float matrix in HBM up to this size
    int pair_mfma = 0;  // WHAT-IF only (built with `make WHATIF=1`): 1 = the AND+popcount tile kernel on the matrix cores
    int finalize_stop = 0;  // profiling only: k_finalize leaves after phase 1..4 (results are then meaningless)
    int finalize_timing = 0;  // profiling only: the s_memtime-stamped instance of k_finalize (same results, per-phase cycles)
    DevBuf phase_cyc;       // 8 x u64 of the last call with finalize_timing
    int nsplit = 0;  // plane-range splits per tile; 0 = auto (aim at >= 16 items per workgroup slot)
    // profiling
    bool profiling = false;
    double pair_ms = 0, fin_ms = 0, prep_ms = 0, sketch_ms = 0, fastx_ms = 0;
    uint32_t pair_launches = 0;
    std::deque<Event> ev_pool;          // timing events, handed out by next_event
    size_t ev_used = 0;

    // ---- state of ONE module each ----
    // sketch waist (sketch.hip): the sequence of a batch, the k_sketch work list of the call in flight, the runs, segments
    // and rows to clear of dsh_sketch_records; dsh_sketch_fastx_batch_async: raw FASTA bytes of a batch, the decoder's
    // tables and scratch (kernels_fastx.hip)
    struct {
        DevBuf seqbuf, workbuf, recbuf;  // (workbuf: dsh_unpermute_blocks_device of abi.hip borrows it for its per-tile deltas)
        Staging work, rec;
        DevBuf rawbuf, fx_tab, fx_summ, fx_state, fx_declen, fx_status;
        DevBuf fx_rec;  // dsh_sketch_fastx_records: the record index and its scratch
        Staging fx;
    } sketch;
    // dsh_dist_threshold* (threshold.hip): a band's per-chunk counts and offsets, the running total, and for the host forms
    // the band's hits and the row pointer on their way out
    struct {
        DevBuf cnt, off, total, col, val, rowptr;
    } thr;
    // dsh_dist_pairs* (pairs.hip): the path's OWN cardinalities (nothing of the dense path's derived state is read or
    // written), a chunk's histograms, the host forms' chunk of the list and of the result, the error words
    // (group_stats.hip and linkage.hip run their pairs through lhs / rhs / out)
    struct {
        DevBuf card, hist, lhs, rhs, out, err;
        Staging list;                 // host forms: a chunk of the list on its way to the device
        int card_estim = -1;          // estimator `card` was computed under (-1: none), dropped by invalidate()
        uint64_t chunk = 1u << 18;    // option pairs_chunk: pairs per launch (scratch is 64 counters per pair of a chunk)
    } pairs;
    // dsh_cluster_* (cluster.hip): parent[n], the root count + error word, a chunk of the caller's edges (or the CSR's row
    // pointer and a chunk of its columns), a seed labelling and the labels of the host forms
    struct {
        DevBuf parent, state, lhs, rhs, rowptr, seed, labels;
        uint64_t chunk = 1u << 20;    // option cluster_chunk: edges per launch of dsh_cluster_pairs / dsh_cluster_csr
    } cc;
    // dsh_greedy_threshold* (greedy.hip): assign[n], the count of representatives and the labels of the host form
    struct {
        DevBuf assign, state, labels;
        DevBuf best;                  // dsh_greedy_extend* in BEST mode (greedy_extend.hip): one 64-bit key per new slot
        uint64_t band_rows = 4096;    // option greedy_band_rows: a band holds at most this many rows (k_greedy_diag's LDS; 1..kGreedyMaxRows)
    } gr;
    // dsh_group_stats* (group_stats.hip): the labels, the per-slot accumulators (cnt, sum, worst key) and per-group medoid
    // keys, the outputs of the host form, and for the pairs route the member CSR
    struct {
        DevBuf labels, acc, grp, out, csr;
        int route = -1;               // option stats_route: -1 auto | 0 dense | 1 pairs
        int route_last = -1;          // (info) the route the last dsh_group_stats* call took
    } gs;
    // dsh_dist_histogram* (hist.hip): the edges, the labels and the call's uint64 counters (the host forms' on their way out)
    struct {
        DevBuf edges, labels, counts;
        int cus = 0;                  // compute units of the device (hipDeviceAttributeMultiprocessorCount), queried once
    } hs;
    // dsh_linkage_* (linkage.hip): the components' tables (comp | rank | moff | coff | mem), the cell matrices of a batch, the
    // state of its members, the labels before they go out, and the count of clusters + the error word
    struct {
        DevBuf tab, cells, nodes, labels, state;
        uint64_t budget = 8ull << 30; // option linkage_budget_bytes: the matrices of a batch of components
        uint32_t lds_max = 4096;      // option linkage_lds_max: components of at most this many members keep their per-row state in LDS
        int partition = 1;            // option linkage_partition: 0 = the whole collection as one component
        int route = -1;               // option linkage_route: -1 auto | 0 dense | 1 pairs
        int route_last = -1;          // (info) the route the last dsh_linkage_threshold* call took
    } lk;
    // dsh_mst* (mst.hip): per slot the best offer of a round, per component root its best key and edge, the edges of the call
    // (lhs | rhs | key, n - 1 each) and their count + the scratch root count of the rounds' labels
    struct {
        DevBuf best, ckey, cedge, elhs, erhs, ekey, state;
        int rounds_last = 0;          // (info) mst_rounds: the rounds of the last call that emitted an edge
        double band_ms = 0;           // (profiling) device time of the last call's k_mst_band launches
    } mst;
    // dsh_dbscan_*, dsh_degree_threshold* (dbscan.hip): per slot its degree and the best offer of a core neighbour, the kinds
    // of the host form, and the counts of clusters and noise + the error word (parent and labels are those of cc)
    struct {
        DevBuf degree, best, kind, state;
    } db;
    // dsh_fold*, dsh_upload_sketches_folded*, dsh_union_groups* (derive.hip): the error word, a chunk of source rows or of
    // folded rows on its way through the device, the groups' CSR and the partial unions of groups cut into chunks
    struct {
        DevBuf err, stage, ptr, mem, dst, part[2], out;
        uint64_t chunk_bytes = (uint64_t)256 << 20;  // option derive_chunk_bytes: source rows staged per step of the host forms
    } derive;
    // dsh_union_curve* (curve.hip): the error word, the orders and the segments' bounds, and per batch the deltas, the
    // segments' start rows, the scan's chunk sums and the counters the estimator reads; the host form's results on their way out
    struct {
        DevBuf err, ord, ptr, delta, start, sums, cnt, card, hist;
        uint64_t scratch_bytes = (uint64_t)256 << 20;  // option curve_scratch_bytes: delta + start rows + counters of a batch of orders
        uint64_t segment = 0;                          // option curve_segment: members per segment, 0 = the planner's (curve_plan.h)
    } curve;
    // multi-GPU exchange (comm.hip, exchange.hip): an RCCL communicator over the ranks' contexts (not owned here:
    // comm_release destroys it while the library is loaded)
    struct {
        ncclComm_t comm = nullptr;
        int rank = 0, world = 1;
        DevBuf gather_full, gather_local;  // dsh_dist_collect: the assembled matrix on the destination rank / this rank's span
        // dsh_exchange_*: on the destination, the row-sorted spans as they arrive and the sources' key order + row offsets
        DevBuf stage, tab;
        Staging tabs;                 // the tables on their way to `tab` (sent on the COPY stream)
        DevBuf place_tab;             // dsh_exchange_place_device's own tables (ctx stream; `tab` belongs to the copy stream)
        bool recv_gated = false;      // (info) the last collect of a destination waited for its tile kernel
        int recv_gate = -1;           // option xch_recv_gate: -1 auto | 0 | 1 (the destination's receives)
        Event ev_place_done;          // the last placement of a collect (the copy stream joins it)
        std::deque<Event> ev_round;   // round q of a collect has arrived (place_stream waits for it)
        double place_ms = 0;          // (profiling) device time of the last dsh_exchange_place_device's placement kernel
        // diagnostics (dsh_diag_spin_*): a kernel that waits like an RCCL receive kernel, on spin_stream
        MappedWord spin_flag;
        bool spin_running = false;
    } xch;
};

namespace dsh {

inline int fail(dsh_ctx *c, int code, const char *fmt, ...)
{
    if (c) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        c->err = buf;
    }
    return code;
}

#define HIPCHK(c, expr)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            (void)hipGetLastError(); /* reported here: a later launch's check must not find it again */ \
            return dsh::fail((c), e_ == hipErrorOutOfMemory ? DSH_ENOMEM : DSH_EIO, "%s: %s",  \
                             #expr, hipGetErrorString(e_));                                    \
        }                                                                                      \
    } while (0)

inline int bind(dsh_ctx *c)
{
    HIPCHK(c, hipSetDevice(c->device));
    return DSH_OK;
}

inline hipEvent_t next_event(dsh_ctx *c)
{
    if (c->ev_used == c->ev_pool.size() && add_event(c->ev_pool, hipEventDefault) != hipSuccess) return nullptr;
    return c->ev_pool[c->ev_used++];
}

// (profiling) the device time of what is enqueued on `st` between the constructor and stop(): two events of the pool.
// Inert -- stop() waits for nothing and leaves `ms` alone -- while profiling is off or where an event could not be made.
struct DeviceTimer {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipStream_t st;
    DeviceTimer(dsh_ctx *c, hipStream_t st_) : st(st_)
    {
        if (!c->profiling) return;
        e0 = next_event(c);
        e1 = next_event(c);
        if (e0 && e1) (void)hipEventRecord(e0, st);
    }
    // waits for the interval's end; its milliseconds replace `ms` or, with `add`, are added to it
    void stop(double &ms, bool add = false)
    {
        if (!e0 || !e1) return;
        (void)hipEventRecord(e1, st);
        (void)hipEventSynchronize(e1);
        float t = 0;
        (void)hipEventElapsedTime(&t, e0, e1);
        ms = add ? ms + t : t;
    }
};

// slots [first, first + cnt) inside [0, total) -- written so that first + cnt cannot wrap
inline bool slots_ok(uint64_t first, uint64_t cnt, uint64_t total) { return first <= total && cnt <= total - first; }

// the sparse counting kernel's table (kernels_sparseplane.hip): a word of it staged in LDS up to p = 15 (option sparse_lds
// = 0: gathered from global memory, the arm the measurements compare against); at p = 16 a word is 256 KiB and the table
// is always gathered
inline int sparse_wordmajor(const dsh_ctx *c) { return c->sparse_lds && c->p <= 15 ? 1 : 0; }
// the table words a workgroup of that LDS placement stages side by side (option sparse_words; 0: one, the measured choice
// at every p -- profiles/sparse4); 0 where the table is gathered
inline int sparse_words_of(const dsh_ctx *c)
{
    if (!sparse_wordmajor(c)) return 0;
    return c->sparse_words > 0 ? c->sparse_words : 1;
}

inline bool use_lockstep(const dsh_ctx *c)
{
    // wherever a plane is at least one chunk (p >= 9): since the kernel needs one barrier per k-row it beats the
    // free-running one at every precision (profiles/r3f/lockstep_ab.jsonl: -5 % at p = 10 ... -17 % at p = 16)
    return !(c->pair_mfma || c->W < (uint32_t)c->kc);
}

// similarity measures rank descending and pass a threshold with v >= t, distances ascending and v <= t (emt2nntype,
// src/dashing.h:268-280): dsh_knn's order and dsh_dist_threshold's direction
inline bool measure_descending(int result_type)
{
    return !(result_type == DSH_MASH_DIST || result_type == DSH_FULL_MASH_DIST || result_type == DSH_CONTAINMENT_DIST ||
             result_type == DSH_FULL_CONTAINMENT_DIST || result_type == DSH_SYMMETRIC_CONTAINMENT_DIST);
}

inline bool whole_sorted(const dsh_ctx *c) { return c->planes_valid && c->lay.whole; }

inline void invalidate(dsh_ctx *c)
{
    c->planes_valid = false;
    c->card_estim = -1;
    c->hk32_valid = false;
    c->pairs.card_estim = -1;
}

// hipStreamWaitValue32 on this device (asked once): what lets the parts of a call announce themselves from inside k_finalize
inline bool device_can_wait_value(dsh_ctx *c)
{
    if (c->can_wait_value < 0) {
        int v = 0;
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeCanUseStreamWaitValue, c->device) != hipSuccess) v = 0;
        c->can_wait_value = v;
        int khz = 0;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess) khz = 0;
        c->wall_clock_khz = khz;
    }
    return c->can_wait_value == 1;
}
// a call with parts will signal them (engine.hip: run_pairs)
inline bool parts_will_signal(dsh_ctx *c) { return !c->finalize_timing && !c->finalize_stop && c->finalize_signal != 0 && device_can_wait_value(c); }

inline void reset_prof(dsh_ctx *c)
{
    c->pair_ms = c->fin_ms = c->prep_ms = 0;
    c->pair_launches = 0;
    c->ev_used = 0;
}

// an entry point that fails after it has enqueued work: leave the stream idle, as every entry point does
inline int drain(dsh_ctx *c, int rc)
{
    (void)hipStreamSynchronize(c->stream);
    (void)hipGetLastError();
    return rc;
}

// what every entry point that reads the resident sketches starts with (reset_prof stays with the entry point: where it
// stands relative to the argument checks differs between them)
inline int enter(dsh_ctx *c)
{
    if (!c) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    if (!c->have_sketches) return fail(c, DSH_ESTATE, "no sketches loaded");
    return DSH_OK;
}

// one pass of the compare path over a set of pairs (engine.hip).  A job starts as one of the two named forms; the rarer
// switches are then set by name where they apply.
struct PairJob {
    int estim = 0, result_type = 0, k = 0;
    int rect = 0;
    int sorted_rows = 0;  // rows (and the output) are in sorted plane-column order (shards)
    int square = 0;       // full triangle, each value written at (i,j) and (j,i) of an n x n matrix
    uint32_t nparts = 0;  // > 0: triangle rows in (at most) this many parts of a key-ordered layout, an event per part
    int rowsorted = 0;    // with nparts: row-sorted parts -- d_out holds the rows in key order (plan.h), not the final span
    int knn = 0;          // band of the key-ordered triangle for the nearest-neighbour selection: d_out = V, d_out2 = Vt
    float *d_out2 = nullptr;
    uint64_t knn_ld = 0, knn_rows = 0;
    int ksinv_double = 0; // 1./k as a double (nndist_loop, src/sketch_and_cmp.h:729) instead of the float of dist_loop (:797)
    uint64_t row_begin = 0, row_end = 0, col_begin = 0, col_end = 0;
    uint64_t base_index = 0;
    float *d_out = nullptr;
    std::vector<uint64_t> extra;  // (with nparts) further row segments {b0, e0, ...} behind row_end: a row set (plan.h)

    // rows [rb, re) of the packed triangle, the value of pair (i, j) at tri(i, j) - base_index of `out`
    static PairJob triangle(int estim, int result_type, int k, uint64_t rb, uint64_t re, uint64_t base_index, void *out)
    {
        PairJob j;
        j.estim = estim, j.result_type = result_type, j.k = k;
        j.row_begin = rb, j.row_end = re;
        j.base_index = base_index;
        j.d_out = (float *)out;
        return j;
    }
    // rows [qb, qe) x columns [rb, re), row-major in `out`
    static PairJob rectangle(int estim, int result_type, int k, uint64_t qb, uint64_t qe, uint64_t rb, uint64_t re, void *out)
    {
        PairJob j;
        j.estim = estim, j.result_type = result_type, j.k = k;
        j.rect = 1;
        j.row_begin = qb, j.row_end = qe, j.col_begin = rb, j.col_end = re;
        j.d_out = (float *)out;
        return j;
    }
};

// cardinalities + thresholds/lists + planes + position index for the current sketch matrix.  want_sorted < 0: whatever
// is cached.  card_only: the per-sketch pass alone.
int prepare(dsh_ctx *c, int estim, int want_sorted, bool card_only = false, uint64_t want_rb = 0,
            uint64_t want_re = ~0ull, uint32_t nparts = 1, int rowsorted = 0, const std::vector<uint64_t> *extra = nullptr);
int run_pairs(dsh_ctx *c, const PairJob &job);

// pairs.hip: the direct pair path over device-resident lists, as dsh_dist_pairs_device runs it
struct PairsQuery {
    int estim, k;
    PairsTypes types;
    uint32_t n_types;
};
int pairs_ensure_cards(dsh_ctx *c, int estim);  // the path's own cardinalities of all n sketches
int pairs_err_begin(dsh_ctx *c);                // the two error words set to "none"
// one chunk: cnt pairs at d_lhs / d_rhs (device), values to d_out[t * out_stride + x]; xbase: the chunk's first pair in the call
int pairs_run_chunk(dsh_ctx *c, const PairsQuery &q, const uint32_t *d_lhs, const uint32_t *d_rhs, uint64_t xbase, uint64_t cnt,
                    float *d_out, uint64_t out_stride);
int pairs_err_end(dsh_ctx *c);                  // the one wait: reads the error words, fails the call on either

// cluster.hip: the union-find of a call on the ctx stream -- parent[n] and the state word set up; the labels and the root count,
// which is the one wait (d_labels: a device buffer, or nullptr for h_labels on the host)
int cc_begin(dsh_ctx *c, uint64_t n);
uint32_t *cc_err(dsh_ctx *c);
uint32_t cc_cap(uint64_t n);
int cc_finish(dsh_ctx *c, uint64_t n, uint32_t *d_labels, uint32_t *h_labels, uint64_t *n_clusters);

// comm.hip: waits for both streams of the communicator's traffic and destroys it (no-op without one)
int comm_release(dsh_ctx *c);
// the world and this context's rank (1, 0 without a communicator), and whether there is a communicator
struct CommWho {
    int world, rank;
    bool comm;
};
CommWho comm_who(const dsh_ctx *c);
// fails with "dsh_comm_init first" unless there is a communicator or the call concerns this rank alone
int need_comm(dsh_ctx *c, bool alone_ok);
// waits for a stream that carries RCCL traffic, with a deadline (DSH_COMM_TIMEOUT_S)
int sync_guarded(dsh_ctx *c, hipStream_t st, const char *what);
int validate_bounds(dsh_ctx *c, uint64_t n, const uint64_t *bounds, int world, int dst);
// one operation of a grouped round: cnt floats from (send) or to `ptr`, with rank `peer`
struct GroupOp {
    bool send;
    void *ptr;
    uint64_t cnt;
    int peer;
};
int post_group(dsh_ctx *c, hipStream_t st, const GroupOp *ops, size_t nops);

}  // namespace dsh
