// kernels.h -- host-callable launchers of the gfx950 kernels (internal to libdashing_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "consts.h"
#include "sketch_plan.h"

namespace dsh {

hipError_t launch_selfhist_card(hipStream_t st, const uint8_t *regs, uint64_t first, uint64_t n, int p, int estim,
                                int emax, int elow, uint32_t *hist, void *exc, uint8_t *excv, uint32_t *exc_n,
                                uint32_t *keys, uint8_t *tailhist, uint32_t *gcnt, uint32_t *sthr, uint32_t scap);
hipError_t launch_card_from_hist(hipStream_t st, const uint32_t *hist, const uint32_t *keys, uint64_t first, uint64_t n, int p,
                                 int estim, double *card);
// position index of every 128-column block of the plane layout (perm == nullptr: identity) and the per-column side
// data of k_finalize in layout order (kernels_compare.hip, k_build_colindex)
// entries held inside a bucket's record: 7 (32-byte records) where a bucket holds ~4 entries and a list at most 256
inline int colindex_inline(int p, uint32_t E) { return p <= 12 && E <= 256 ? 7 : 3; }
struct ColIndexLaunch {
    const void *exc;          // per sketch (original index): listed positions, values, counts, keys, cardinalities, tail histograms
    const uint8_t *excv;
    const uint32_t *exc_n, *keys;
    const double *card;
    const uint8_t *tailhist;
    const uint32_t *perm;
    uint64_t ncols;
    int p;
    uint32_t nblocks, nbuckets, ent_stride, E;  // E = entries of a compact list row (emax + elow)
    uint32_t *rec;            // [nblocks][nbuckets][colindex_inline(p, E) + 1]
    uint32_t *ent;            // [nblocks][ent_stride]
    uint32_t *nS, *keyS;      // [Npad]
    double *cardS;            // [Npad]
    uint8_t *thS;             // [Npad][64]
    uint32_t *rl;             // [Npad][E]
};
hipError_t launch_build_colindex(hipStream_t st, const ColIndexLaunch &c);
hipError_t launch_transform(hipStream_t st, const uint8_t *regs, uint64_t n, int p, int vlo,
                            uint32_t P, uint32_t W, uint32_t Npad, uint32_t *planes,
                            const uint32_t *perm);
hipError_t launch_pair_counts(hipStream_t st, int kc, int cum_bytes, const uint32_t *planes,
                              uint32_t Npad, uint32_t Kpad, uint32_t W, uint32_t P,
                              const uint4 *tiles, const uint4 *items, uint32_t nitems, void *cum,
                              uint64_t nslots);

// sparse outer planes (kernels_sparseplane.hip; plan.h, Tuning::sparse_planes, sparse_sided).  launch_sparse_build: for each
// of the nslabs {block, plane | plan::kSpSlab* flags} of `slabs`, from that plane's words of the bit-plane matrix,
// tab[slab][2^p][4] (bit j of a position's 128: column j of the block is in the slab's set there -- its register >= the
// plane's threshold, or with kSpSlabA < it), lists[slab][128][cap] (every column's such positions, 16-bit; none for a
// kSpSlabTableOnly slab) and len[slab][128] (the size of every set; cleared here first).  cap: a multiple of 8.  wordmajor: the table as
// tab[slab][4][2^p], which the LDS placement of the counting kernel stages a word of (2^p <= 2^15); the two launchers of
// a call take the same value.
hipError_t launch_sparse_build(hipStream_t st, const uint32_t *planes, uint32_t Npad, uint32_t W, uint64_t ncols, const uint2 *slabs,
                               uint32_t nslabs, uint32_t cap, int wordmajor, uint32_t *tab, uint16_t *lists, uint32_t *len);
// one workgroup per item {tile index in band, plane | plan::kSpItem* flags, slab of the row block, slab of the column block}:
// the plane's C(v) of the tile's 128 x 128 pairs, stored where the tile kernel stores it; m = 2^p.  The flags name the
// polarities of the list side and the table side, and whether the list side is the column block (a transposed item).
// run >= 1 (wordmajor only; the gathered kernel ignores it): a workgroup of the LDS placement takes that many items of an
// XCD residue one behind the other and stages the table where it changes (plan.h, sparse_table_fills); 1 = one item each.
// words = 1 | 2 (wordmajor only): the table words a workgroup stages side by side; 2 needs 2^p <= 2^14, refused otherwise
hipError_t launch_sparse_count(hipStream_t st, int cum_bytes, const uint4 *items, uint32_t nitems, uint32_t run, int wordmajor, int words,
                               const uint32_t *tab, const uint16_t *lists, const uint32_t *len, uint32_t cap, uint32_t m, void *cum,
                               uint64_t nslots);

// what-if variant on the matrix cores (option "pair_mfma"; never the default: the north star excludes MFMA)
// the same arithmetic with the waves of a SIMD kept in one instruction class: workgroups of 256 * groups threads with
// `groups` items each (2 | 3).  Three groups exist for kc = 16 only (LDS): groups = 3 with kc = 32 is refused with
// hipErrorInvalidValue.
hipError_t launch_pair_counts_lockstep(hipStream_t st, int kc, int groups, int cum_bytes, const uint32_t *planes,
                                       uint32_t Npad, uint32_t Kpad, uint32_t W, uint32_t P, const uint4 *tiles,
                                       const uint4 *items, uint32_t nitems, uint32_t nfrag, void *cum, uint64_t nslots);
hipError_t launch_pair_counts_mfma(hipStream_t st, int kc, int cum_bytes, const uint32_t *planes,
                                   uint32_t Npad, uint32_t Kpad, uint32_t W, uint32_t P,
                                   const uint4 *tiles, const uint4 *items, uint32_t nitems, void *cum,
                                   uint64_t nslots);

// the by-value argument of k_finalize / k_finalize_signal (kernels_compare.hip): filled by run_pairs (engine.hip), ntiles
// by launch_finalize.  Member order and types are the kernels' argument layout: its ~70 dwords already press on the
// scalar registers (kernels_compare.hip, finalize_block), so nothing is added or reordered here in passing.
struct FinalizeArgs {
    const void *cum;
    uint64_t nslots;       // distance between two planes of cum (pair slots of the band)
    const uint4 *tiles;    // {row block, col block, plane begin, plane end} per tile
    const uint32_t *perm;  // plane-matrix column -> sketch index (nullptr: identity)
    // row-sorted parts (plan.h): the output buffer holds the wanted rows in KEY order, the row at layout position s
    // starting at rowoff[s]; nullptr: the rows' span of the packed triangle in final order
    const uint64_t *rowoff;
    int hist_bins;  // histogram columns allocated per lane (>= the value span of any tile of the launch)
    int pbase;  // plane pl is the threshold v = pbase + 1 + pl
    int p;
    int estim;
    int result_type;
    double ksinv;
    // per COLUMN of the layout, in layout order (k_build_colindex): nothing below waits for the permutation
    const uint32_t *nS;       // [Npad] listed registers of the column's sketch
    const uint32_t *keyS;     // [Npad] hi << 18 | T << 12 | L << 6 | lo
    const double *cardS;      // [Npad]
    const uint8_t *thS;       // [Npad][64]: how many listed registers have each value above the sketch's T
    const uint32_t *rl;       // [Npad][E]: the listed registers, position << 8 | value
    uint32_t E;
    const uint32_t *cidx_rec; // position index of the column blocks: [blocks][nbuckets][RK + 1] records
    const uint32_t *cidx_ent; // [blocks][ent_stride] all entries in bucket order (buckets with more than RK entries)
    uint32_t nbuckets, ent_stride;
    uint64_t n;      // sketches in the collection = dimension of the output matrix
    uint64_t ncols;  // real columns of the plane matrix (a sub-collection when only a row range is wanted)
    // triangle mode: rows [row_begin,row_end) (original indices), out index = tri(i,j) - base_index
    // rect mode (rect != 0): i in [row_begin,row_end) x j in [col_begin,col_end), row-major
    int rect;
    // sorted_out != 0 (triangle mode only): rows and the output index are in plane-column
    // (sorted) order instead of original sketch order -- used for multi-GPU shards, whose spans
    // are gathered first and un-permuted once (k_unpermute)
    int sorted_out;
    // square != 0 (triangle tiles, all rows): every pair is written at BOTH out[i*n+j] and
    // out[j*n+i] of an n x n matrix (the all-vs-all nearest-neighbour path: each pair computed once)
    int square;
    // knn != 0 (whole key-ordered layout, rows = plane columns [row_begin,row_end) like sorted_out): the pair (si, sj),
    // si < sj, is written twice -- out[(si - row_begin) * knn_ld + sj] is a candidate of row si, out2[sj * knn_rows +
    // (si - row_begin)] a candidate of row sj -- for the band-wise nearest-neighbour selection (k_topk_merge)
    int knn;
    float *out2;
    uint64_t knn_ld, knn_rows;
    int stop;             // profiling only (option "finalize_stop"): leave after phase 1..4 with a dummy store
    uint32_t ntiles;      // tiles of this launch
    unsigned long long *phase_cyc;  // profiling only (TIMED instances): shader-clock cycles per phase, summed over waves
    uint64_t row_begin, row_end, col_begin, col_end;
    uint64_t base_index;
    float *out;
    // part signalling (k_finalize_signal; kernels.h kSig*): counters and flags of the call's parts; the generation value
    // that marks a part final and the stamp switch live in the block itself (two kernel arguments fewer)
    uint32_t *sig;
};
static_assert(sizeof(FinalizeArgs) == 272, "the kernel argument of k_finalize changed its layout");
// a launch of k_finalize over a band of tiles or a segment of it (a.cum / a.tiles point at its first tile): the kernel's
// arguments and the two host-only quantities that pick the instance and size the launch
struct FinalizeLaunch {
    FinalizeArgs a;
    int cum_bytes;    // 2 or 4
    uint64_t nslots;  // pair slots to finalize (a.nslots: those of the whole band)
};
hipError_t launch_finalize(hipStream_t st, const FinalizeLaunch &f);
// the signal block of a call with parts, in 32-bit words: per part a flag (= the generation of the call that completed
// it), a count of finished tiles, the tiles it holds in all, a 64-bit wall-clock stamp of its completion; the stamp of the
// call's start; per tile of the band in flight a count of finished rows
constexpr uint32_t kSigPartFlag = 0, kSigPartCnt = kSigMaxParts, kSigPartTotal = 2 * kSigMaxParts,
                   kSigGen = 3 * kSigMaxParts, kSigStamp = kSigGen + 1,  // (uploaded with the totals: kSigMaxParts + 2 words)
                   kSigPartTime = 3 * kSigMaxParts + 2, kSigT0 = 5 * kSigMaxParts + 2, kSigTileCnt = 5 * kSigMaxParts + 4,
                   kSigWords = kSigTileCnt + 65536;
// (k_upload_segs) up to four uploads from page-locked staging in one launch
struct UploadSeg {
    uint32_t *dst;
    const uint32_t *src;
    uint64_t nwords;
};
struct UploadSegs {
    UploadSeg s[4];
    void add(uint32_t &n, void *dst, const void *src, size_t bytes)
    {
        if (!bytes) return;
        s[n].dst = (uint32_t *)dst, s[n].src = (const uint32_t *)src, s[n].nwords = (bytes + 3) / 4;
        ++n;
    }
};
hipError_t launch_upload_segs(hipStream_t st, const UploadSegs &u, uint32_t nseg);
hipError_t launch_wall_stamp(hipStream_t st, unsigned long long *out);
// ---- kernels_exchange.hip: row placement at the destination of an exchange, the older shard scheme's un-permute, the
// kernels of the one-GPU diagnostics
// (k_rows_place) the rows of one source's part in a round of the exchange: positions [pos0, pos0 + nrows) of its key order
struct PlaceEnt {
    const float *src;         // the source's staged buffer
    const uint32_t *order;    // its key order (original row of every position)
    const uint64_t *rowoff;   // where the row at a position starts in the buffer
    uint64_t pos0;
    uint32_t row0, nrows;     // the blocks [row0, row0 + nrows) of the launch
};
hipError_t launch_rows_place(hipStream_t st, const PlaceEnt *ent, uint32_t nent, uint32_t total_rows, float *out, uint64_t n);
// rows [pos0, pos1) of a row-sorted buffer (order[s] = original row, rowoff[s] = its offset) into the packed triangle
hipError_t launch_row_place(hipStream_t st, const float *src, float *out, const uint32_t *order, const uint64_t *rowoff,
                            uint64_t pos0, uint64_t pos1, uint64_t n);
hipError_t launch_unpermute_staged(hipStream_t st, const float *in, const uint32_t *inv,
                                   const int64_t *rowdelta, uint64_t n, float *out);
// destination-driven (coalesced writes, gathered reads through inv, the inverse of perm)
hipError_t launch_unpermute(hipStream_t st, const float *in, const uint32_t *inv, uint64_t n, float *out);
// (diagnostics) cnt floats copied by plain loads and stores; a kernel that waits on a mapped word of host memory
hipError_t launch_probe_copy(hipStream_t st, const float *src, float *dst, uint64_t cnt);
hipError_t launch_diag_spin(hipStream_t st, uint32_t nblocks, uint32_t threads, uint32_t lds_bytes, const uint32_t *flag, unsigned long long max_ticks);

// ---- knn.hip: nearest-neighbour selection (k_topk: one pass over a matrix of values)
hipError_t launch_topk(hipStream_t st, const float *vals, uint64_t rows, uint64_t ncols,
                       uint64_t row0, uint64_t col0, int descending, uint32_t nn,
                       int exclude_self, uint32_t *idx_out, float *val_out);

// band-wise nearest neighbours (no n x n matrix; k_topk_merge, k_fill_knn_state): running lists idx/val[n][nn] by sketch index
hipError_t launch_knn_state_init(hipStream_t st, uint32_t *idx, float *val, uint64_t cnt, int descending);
hipError_t launch_topk_merge(hipStream_t st, const float *vals, uint64_t ld, int mode, uint64_t b0, uint64_t rows,
                             uint64_t ncols, const uint32_t *perm, int descending, uint32_t nn, uint32_t *st_idx,
                             float *st_val);

// thresholded output (kernels_threshold.hip, threshold.hip): the rows of a band buffer -- rows [row0, row0 + rows) of the
// packed triangle of n sketches back to back (row i: n - 1 - i values, columns i + 1 ...), or rows x ncols of a rectangle
// (columns col0 ...) -- each cut into nchunks chunks of kThrChunk values (consts.h; nchunks covers the longest row)
struct ThrRows {
    int rect;
    uint64_t n, row0;      // triangle
    uint64_t ncols, col0;  // rectangle
    uint64_t rows;
    uint32_t nchunks;
};
// the grid of the kernels that walk it (thr_walk.h): block (r, y) holds the chunks 4 y .. 4 y + 3 of band row r
inline dim3 thr_grid(const ThrRows &g) { return dim3((uint32_t)g.rows, (g.nchunks + 3) / 4); }
// cnt[rows * nchunks]: hits per chunk (similarity measures pass with v >= t, distances with v <= t; NaN never)
hipError_t launch_thr_count(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *cnt);
// off[m + 1] = *total + exclusive scan of cnt[m] (m = rows * nchunks), row_ptr[r] = off[r * nchunks], *total = off[m]
hipError_t launch_thr_scan(hipStream_t st, const uint32_t *cnt, uint64_t m, uint32_t nchunks, uint64_t *off, uint64_t *row_ptr,
                           uint64_t *total);
// hit number h (in row-major, column-ascending order) goes to col/val[h - sub] if that is below cap
hipError_t launch_thr_emit(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, const uint64_t *off,
                           uint64_t sub, uint64_t cap, uint32_t *col, float *val);

// threshold clusters (kernels_cluster.hip, cluster.hip): a union-find over parent[n] with parent[x] <= x (uf.h).  cap bounds
// every loop (n + 1); err is one device word that a step-bound overrun sets (it starts at 0)
hipError_t launch_cc_init(hipStream_t st, uint32_t *parent, uint64_t n);
hipError_t launch_cc_seed(hipStream_t st, uint32_t *parent, const uint32_t *labels_in, uint64_t n, uint32_t cap, uint32_t *err);
hipError_t launch_cc_edges(hipStream_t st, uint32_t *parent, const uint32_t *lhs, const uint32_t *rhs, uint64_t n_edges, uint64_t n,
                           uint32_t cap, uint32_t *err);
// hits [h0, h0 + cnt) of a CSR (row_ptr [rows + 1] whole on the device, counted from 0; col = the columns of THESE hits):
// hit h of row r unites row_begin + r with its column
hipError_t launch_cc_csr(hipStream_t st, uint32_t *parent, const uint64_t *row_ptr, uint64_t rows, uint64_t row_begin,
                         const uint32_t *col, uint64_t h0, uint64_t cnt, uint64_t n, uint32_t cap, uint32_t *err);
// a band of triangle rows as launch_thr_count takes it: every passing value unites its row and its column
hipError_t launch_cc_band(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *parent, uint32_t cap,
                          uint32_t *err);
// labels[x] = root of x (the smallest member of its component), *n_roots += the roots (the caller zeroes it)
hipError_t launch_cc_labels(hipStream_t st, uint32_t *parent, uint64_t n, uint32_t cap, uint32_t *labels, uint64_t *n_roots, uint32_t *err);

// greedy representatives (kernels_greedy.hip, greedy.hip): assign[n] starts as assign[x] = x (launch_cc_init) and only
// decreases; assign[x] < x: x is covered by that representative.  Per band of triangle rows, in stream order:
constexpr uint32_t kGreedyMaxRows = 8192;  // rows of a band: k_greedy_diag keeps their entries in LDS (32 KiB)
// the band's rows among themselves (g.rows <= kGreedyMaxRows): afterwards assign[row0 .. row0 + rows) is final
hipError_t launch_greedy_diag(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *assign);
// every representative row of the band lowers assign[j] to itself for its passing columns j >= row0 + rows
hipError_t launch_greedy_band(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *assign);
// after the last band: labels[x] = assign[x], *n_reps += the x with assign[x] == x (the caller zeroes it)
hipError_t launch_greedy_labels(hipStream_t st, const uint32_t *assign, uint64_t n, uint32_t *labels, uint64_t *n_reps);
// dsh_greedy_extend* (greedy_extend.hip): slots below first_new keep the caller's labels; best[n - first_new] (BEST mode,
// else nullptr) starts as 0 and holds per new slot the largest key (value, then smaller slot) of a representative that hits it.
// Rows of a rectangle [g.row0, g.row0 + g.rows) x [g.col0 = first_new, n): every row that is a representative lowers
// assign[j] to itself and (best != nullptr) raises best[j - first_new] for its passing columns
hipError_t launch_greedy_rect(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *assign, uint64_t *best);
// a band of triangle rows at or behind first_new, after launch_greedy_diag and IN THE PLACE of launch_greedy_band: its
// representative rows raise best for all their passing columns and lower assign for those >= row0 + rows
hipError_t launch_greedy_best(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *assign, uint64_t *best,
                              uint64_t first_new);
// labels[x] = assign[x], or for a covered x >= first_new with best != nullptr the slot its key names; *n_reps += the x with labels[x] == x
hipError_t launch_greedy_extend_labels(hipStream_t st, const uint32_t *assign, const uint64_t *best, uint64_t first_new, uint64_t n,
                                       uint32_t *labels, uint64_t *n_reps);

// statistics of a labelling (kernels_group.hip, group_stats.hip): per slot the included pairs inside its group, the sum of
// their values in 2^-30 units and the key of the worst one (0: none); the caller zeroes all three
struct GsAccum {
    uint32_t *cnt;
    uint64_t *sum;
    uint32_t *wkey;
};
// a band of triangle rows as launch_thr_count takes it, labels[n] on the device: what the band's pairs add to their ROWS ...
hipError_t launch_gs_rows(hipStream_t st, const float *vals, const ThrRows &g, const uint32_t *labels, int descending, const GsAccum &a);
// ... and to their COLUMNS
hipError_t launch_gs_cols(hipStream_t st, const float *vals, const ThrRows &g, const uint32_t *labels, int descending, const GsAccum &a);
// the intra-group pairs [x0, x0 + cnt) of a member CSR over the groups of at least two members: ppre[ngroups + 1] pairs before
// each group, moff[ngroups + 1] its first member in mem (slots ascending inside a group); lhs = the larger slot
hipError_t launch_gs_enum(hipStream_t st, const uint64_t *ppre, const uint32_t *moff, const uint32_t *mem, uint64_t ngroups, uint64_t x0,
                          uint64_t cnt, uint32_t *lhs, uint32_t *rhs);
// the values of n_pairs pairs folded into both ends
hipError_t launch_gs_pairs(hipStream_t st, const uint32_t *lhs, const uint32_t *rhs, const float *vals, uint64_t n_pairs, uint64_t n,
                           int descending, const GsAccum &a);
// the medoid of every group (g_cnt, g_sum zeroed, g_slot all ones by the caller, [n] each, indexed by label) and the four
// outputs, each written only where its pointer is not null
hipError_t launch_gs_finish(hipStream_t st, const uint32_t *labels, uint64_t n, int descending, const GsAccum &a, uint32_t *g_cnt,
                            uint64_t *g_sum, uint32_t *g_slot, uint32_t *medoid_out, uint32_t *cnt_out, int64_t *sum_out, float *worst_out);

// linkage clusters at a threshold (kernels_linkage.hip, linkage.hip, linkage.h): the components of at least two members as a
// member CSR on the device, and the batch of them whose m x m cell matrices (uint32 keys, int64 sums for AVERAGE) are resident
struct LkComps {
    const uint32_t *comp;  // [n] the component of a slot, 0xFFFFFFFF: none (a singleton)
    const uint32_t *rank;  // [n] its index inside the component (its rank in slot order)
    const uint32_t *moff;  // [components + 1] the component's first member in mem
    const uint64_t *coff;  // [components] the first cell of its matrix in the scratch of its batch
    const uint32_t *mem;   // the members, slots ascending inside a component
};
struct LkBatch {
    uint32_t c0, c1;   // the components of the batch
    void *cells;       // their matrices
    uint64_t ncells;   // cells the scratch holds: no store goes beyond
    void *state;       // nnv | size | nn | root | alive for the batch's members (the components above lds_max use theirs)
    uint32_t mbase;    // moff[c0]
    uint32_t members;  // moff[c1] - moff[c0]
};
// a band of triangle rows as launch_thr_count takes it: the values inside a component of the batch become cells
hipError_t launch_lk_fill_band(hipStream_t st, int linkage, const float *vals, const ThrRows &g, const LkComps &C, const LkBatch &B, int descending);
// the same for the values of cnt pairs of slots below n
hipError_t launch_lk_fill_pairs(hipStream_t st, int linkage, const uint32_t *lhs, const uint32_t *rhs, const float *vals, uint64_t cnt,
                                uint64_t n, const LkComps &C, const LkBatch &B, int descending);
// one workgroup per component of the batch: labels[member] = the smallest slot of its final cluster.  lds_members: the largest
// component of the batch that is at most lds_max; cap bounds every loop (the largest m + 1); err: one device word, starts at 0
hipError_t launch_linkage(hipStream_t st, int linkage, const LkComps &C, const LkBatch &B, float threshold, int descending, uint32_t lds_max,
                          uint32_t lds_members, uint32_t cap, uint32_t *labels, uint32_t *err);
size_t linkage_lds_bytes(int linkage, uint32_t m);  // LDS of a workgroup of k_linkage whose state holds m members

// minimum spanning tree of the pair values (kernels_mst.hip, mst.hip, mst.h): one Borůvka round over labels[n] (launch_cc_labels),
// best_v[n] and ckey[n] zeroed and cedge[n] all ones by the caller
struct MstEdges {
    uint32_t *lhs, *rhs, *key;  // [room] the edges of the call so far, in arbitrary order
    unsigned long long *count;  // how many
    uint64_t room;              // n - 1: no store goes beyond
};
// a band of triangle rows as launch_thr_count takes it: every value that passes the cutoff between two components offers
// itself to best_v of both ends
hipError_t launch_mst_band(hipStream_t st, const float *vals, const ThrRows &g, float cutoff, int descending, const uint32_t *labels,
                           uint64_t *best_v);
// per component root: ckey = the best key among its members' offers, cedge = the smallest (i << 32 | j) that holds it
hipError_t launch_mst_pick(hipStream_t st, const uint64_t *best_v, const uint32_t *labels, uint32_t *ckey, uint64_t *cedge, uint64_t n);
// the roots' edges appended to e (a mutual choice once) and their ends united in parent (cap, err: as launch_cc_edges)
hipError_t launch_mst_emit(hipStream_t st, const uint32_t *labels, const uint32_t *ckey, const uint64_t *cedge, uint64_t n, uint32_t *parent,
                           uint32_t cap, uint32_t *err, const MstEdges &e);

// density clusters at a threshold (kernels_dbscan.hip, dbscan.hip): a band of triangle rows as launch_thr_count takes it
constexpr uint32_t kDbSlab = 512;  // band rows a thread of k_db_deg_cols walks
// walk 1: every passing value adds one to degree[] of its row and of its column (degree zeroed by the caller)
hipError_t launch_db_degree(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, uint32_t *degree);
// walk 2, degree[n] final: a passing value between two cores (degree + 1 >= min_pts) unites them in parent (cap, err: as
// launch_cc_band); between a core c and a non-core b it offers (hi << 32 | ~c) to best[b] (zeroed by the caller) under a
// maximum, hi = the value's key (assign_best) or 1
hipError_t launch_db_band(hipStream_t st, const float *vals, const ThrRows &g, float t, int descending, const uint32_t *degree,
                          uint32_t min_pts, int assign_best, uint32_t *parent, uint32_t cap, uint32_t *err, uint64_t *best);
// labels[x]: a core's root, a border's core's root, a noise point itself; kind_out / degree_out where not null; *n_clusters +=
// the cores that are their own label, *n_noise += the noise points (the caller zeroes both)
hipError_t launch_db_labels(hipStream_t st, uint32_t *parent, uint64_t n, uint32_t cap, const uint32_t *degree, const uint64_t *best,
                            uint32_t min_pts, uint32_t *labels, uint8_t *kind_out, uint32_t *degree_out, uint64_t *n_clusters,
                            uint64_t *n_noise, uint32_t *err);

// value histograms (kernels_hist.hip, hist.hip): a band of triangle or rectangle rows as launch_thr_count takes it, counted
// into counts[planes][n_edges + 2] (device, 64-bit adds: the caller zeroes it) over the n_edges strictly increasing edges at
// d_edges (device); class(v) = the edges that pass v as a threshold would, NaN = n_edges + 1.  labels == nullptr: one plane;
// else labels[n] on the device and plane = (label of the row's slot != label of the column's slot)
// cus: the compute units of the device (the residency bound of plan::hist_grid)
hipError_t launch_hist(hipStream_t st, const float *vals, const ThrRows &g, const float *d_edges, uint32_t n_edges, const uint32_t *labels,
                       int descending, uint32_t cus, uint64_t *counts);
size_t hist_lds_bytes(uint32_t n_edges, int planes);  // LDS of a workgroup of k_hist

// explicit pair lists (kernels_pairs.hip, pairs.hip): histograms are [cnt][64] counters, uint16 for p <= kPairsMaxP16
// (a bin holds at most 2^p), uint32 above
constexpr int kPairsMaxP16 = 15;
struct PairsTypes {
    int t[9];
};
// hist[x] = histogram of max(sketch lhs[x], sketch rhs[x]) for x in [0, cnt); lhs == nullptr: of sketch first + x alone.
// err (device, 2 x u64, may be nullptr with lhs == nullptr): [0] = min over the pairs naming a slot >= n of xbase + x,
// [1] = min over the named sketches that hold an out-of-range register; the caller initialises both to ~0
hipError_t launch_pairs_hist(hipStream_t st, const uint8_t *regs, uint64_t n, int p, const uint32_t *lhs, const uint32_t *rhs,
                             uint64_t first, uint64_t xbase, uint64_t cnt, void *hist, unsigned long long *err);
// card[first + x] = estimate of hist[x], x in [0, cnt)
hipError_t launch_pairs_card(hipStream_t st, const void *hist, uint64_t first, uint64_t cnt, int p, int estim, double *card);
// out[t * out_stride + x] = float(result_cmp(card[lhs[x]], card[rhs[x]], estimate of hist[x], types.t[t], ksinv))
hipError_t launch_pairs_finish(hipStream_t st, const void *hist, const uint32_t *lhs, const uint32_t *rhs, uint64_t n, uint64_t cnt,
                               int p, int estim, const double *card, const PairsTypes &types, uint32_t n_types, double ksinv,
                               float *out, uint64_t out_stride);

// derived sketches (kernels_derive.hip, derive.hip)
// rows [n][2^ps] at src (any alignment) folded to [n][2^pd] at dst (any alignment), pd <= ps; *err (device, starts at ~0) =
// min over the rows that hold a register above 64 - ps + 1 of row0 + row
hipError_t launch_fold(hipStream_t st, const uint8_t *src, uint64_t n, int ps, int pd, uint64_t row0, uint8_t *dst,
                       unsigned long long *err);
// row v in [0, nv) = byte-wise max of the rows mem[ptr[v] .. ptr[v + 1]) of src (mem == nullptr: the rows ptr[v] .. ptr[v + 1)
// themselves), written to row dst[v] of out_a, or with bit 31 of dst[v] set to row dst[v] & 0x7FFFFFFF of out_b
// (dst == nullptr: row v of out_a).  src, out_b 16-byte aligned; out_a any alignment.
hipError_t launch_union_groups(hipStream_t st, const uint8_t *src, int p, const uint64_t *ptr, const uint32_t *mem,
                               const uint32_t *dst, uint64_t nv, uint8_t *out_a, uint8_t *out_b);

// union growth curves (kernels_curve.hip, curve.hip); the cut into segments and batches is curve_plan.h's
constexpr int kCurveLoadsInFlight = 4;     // rows whose loads a lane of k_curve_walk has in flight
constexpr uint32_t kCurveScanChunk = 128;  // steps per chunk of k_curve_scan* (curve_plan.h: kScanChunk)
// the `orders` orders ord[o * len + j] (slots below n; others are skipped), each cut into nseg segments of S members:
// delta[o * len + j][64] (int32, zeroed by the caller) gets -1 at the bin a register leaves and +1 at the bin it reaches at
// step j.  start (nseg > 1): row o * nseg + s = the union of the members in front of segment s (launch_curve_starts).
// *err (device, starts at ~0) = min over the members that hold a register above 64 - p + 1.
hipError_t launch_curve_walk(hipStream_t st, const uint8_t *regs, uint64_t n, int p, const uint32_t *ord, uint64_t len, uint64_t S,
                             uint64_t nseg, uint64_t orders, const uint8_t *start, int *delta, unsigned long long *err);
// rows o * nseg + s of start, s = 0 .. nseg - 1: the segments' unions on entry, the unions of the segments in front of each on exit
hipError_t launch_curve_starts(hipStream_t st, uint8_t *start, int p, uint64_t nseg, uint64_t orders);
// cnt[o * len + i][64] = the histogram of the union of the first i + 1 members of order o: 2^p in bin 0 plus the deltas up to
// step i, in launch_pairs_card's layout (uint16 for p <= kPairsMaxP16, uint32 above); the same as uint32 to hist where not
// null.  sums: scratch, [orders * ceil(len / kCurveScanChunk)][64] int32 (not read where that is one chunk per order).
hipError_t launch_curve_scan(hipStream_t st, const int *delta, int *sums, uint64_t len, uint64_t orders, int p, void *cnt, uint32_t *hist);

// in-order upload of a small page-locked host buffer by a kernel (no runtime copy on the ctx stream)
hipError_t launch_upload(hipStream_t st, void *dst, const void *src_pinned, size_t bytes);

// sketch path: the lists the host fills (SketchWork, RecRun, RecSeg, FastxChunk, FastxGenome) are sketch_plan.h's
hipError_t launch_sketch(hipStream_t st, const uint8_t *seq, const SketchWork *work,
                         uint32_t nwork, int k, int p, int canon, uint8_t *regs);
// per-record sketches (k_sketch_records): a workgroup per run; segs holds the planner's RecSeg entries
static_assert(sizeof(RecSeg) == sizeof(uint2) && alignof(RecSeg) <= alignof(uint2), "k_sketch_records reads a RecSeg as a uint2");
hipError_t launch_sketch_records(hipStream_t st, const uint8_t *seq, const RecRun *runs, uint32_t nruns, const uint2 *segs,
                                 int k, int p, int canon, uint8_t *regs);
// zero the rows slots[0 .. nslots) of the matrix (2^p bytes each)
hipError_t launch_zero_rows(hipStream_t st, const uint32_t *slots, uint32_t nslots, int p, uint8_t *regs);

// FASTA text -> clean base stream on the device (kernels_fastx.hip)
struct FastxSumm {  // what a chunk tells the per-genome scan (kernels_fastx.hip, k_fastx_scan)
    uint32_t fn, bad8;
    uint32_t a[4], b[4];
};
// summ [nchunks], state [nchunks] uint4, declen [ngenomes], status and fingerprint [ngenomes] (both zeroed by the caller;
// status != 0 afterwards: not what its format promises, nothing emitted)
hipError_t launch_fastx_decode(hipStream_t st, const uint8_t *raw, const FastxChunk *chunks, uint32_t nchunks,
                               const FastxGenome *genomes, uint32_t ngenomes, FastxSumm *summ, uint4 *state, uint64_t *declen,
                               uint32_t *status, unsigned long long *fingerprint, uint8_t *out);
// The record index (dsh_sketch_fastx_records): in the decoded stream every record begins with one
// marker byte -- FASTA a header's first byte, FASTQ the newline that ends a header line, both emitted as 'N' -- which a
// literal N of a sequence cannot be told from afterwards, so separate instances of the three kernels write them down.  FastxSumm and
// the genome path's kernels stay as they are.  Positions count from the start of the raw / decoded buffer.
struct FastxRecIndex {
    uint32_t *cnt;         // [nchunks][3] scratch: a FASTA chunk's markers under each carry (pass A -> B)
    uint32_t *nrec;        // [ngenomes][2]: the file's markers; the carry behind its last byte (FASTQ: the line index it ends on)
    const uint64_t *rec0;  // [ngenomes + 1] a file's first entry and, one further, the end of its entries; NULL: count only
    uint64_t *dpos, *rpos; // [rec0[ngenomes]] a marker's place in the decoded and in the raw buffer
};
hipError_t launch_fastx_decode_records(hipStream_t st, const uint8_t *raw, const FastxChunk *chunks, uint32_t nchunks,
                                       const FastxGenome *genomes, uint32_t ngenomes, FastxSumm *summ, uint4 *state, uint64_t *declen,
                                       uint32_t *status, unsigned long long *fingerprint, uint8_t *out, const FastxRecIndex &ix);

// dsh_preload: load the code objects of the kernel translation units now (else: at the first launch from each)
hipError_t preload_compare_kernels();
hipError_t preload_hist_kernels();      // (part of the compare set)
hipError_t preload_sparseplane_kernels();  // (part of the compare set: kernels_sparseplane.hip)
hipError_t preload_knn_kernels();       // (part of the compare set: knn.hip)
hipError_t preload_exchange_kernels();  // (part of the compare set: kernels_exchange.hip)
hipError_t preload_fastx_kernels();
hipError_t preload_sketch_kernels();

// hipFuncAttributeMaxDynamicSharedMemorySize of a kernel, raised once per (kernel, device) instead of on every launch
// (ADVICE r4): remembers the largest size granted so far and only calls the runtime for a larger one.
hipError_t ensure_dynamic_lds(const void *kernel, size_t bytes);

}  // namespace dsh
