/*
 * dashing_hip.h -- C-ABI of libdashing_hip.so: dashing's HLL sketch-and-compare hot path on
 * MI355X (gfx950).  Plain pointers and sizes only; no C++/torch types cross this boundary.
 *
 * dashing (the reference, /root/reference) has no plugin/FFI interface for this path: it is
 * C++ templates instantiated per sketch type.  Each entry point below replaces one of the two
 * loop bodies ("waists") of the reference, cited file:line; INTEGRATION.md shows the
 * reference-side glue a maintainer would add.
 *
 * Conventions
 *   - every function returns DSH_OK (0) or a negative errno-style code; no exceptions cross
 *     the boundary; dsh_last_error(ctx) gives a human-readable message for the last failure.
 *   - the caller owns all host memory; the library owns device memory behind dsh_ctx.
 *   - one dsh_ctx per GPU; a ctx is not thread-safe, different ctxs are independent.
 *   - there is NO CPU fallback: with no gfx950 device dsh_create fails with DSH_ENODEV.
 *   - register arrays are dashing's: uint8_t[2^p] per sketch, row-major [n][2^p].
 *   - distances are float32 in the packed upper-triangular order of
 *     distmat/distmat.h:260-264: index(i,j) = i*(2n-i-1)/2 + j-(i+1), i<j.
 */
#ifndef DASHING_HIP_H_
#define DASHING_HIP_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSH_OK 0
#define DSH_EINVAL (-22)  /* bad argument */
#define DSH_ENOMEM (-12)  /* host or device allocation failed */
#define DSH_ENODEV (-19)  /* no usable gfx950 device */
#define DSH_EIO (-5)      /* HIP runtime error / file error */
#define DSH_ESTATE (-11)  /* call sequence error (e.g. dist before sketches are loaded) */
#define DSH_ERANGE (-34)  /* the result does not fit the capacity the caller gave (dsh_dist_threshold_device) */

/* sketch::hll::EstimationMethod values selected by dist_main, src/distmain.cpp:37,59-62
 * (-E ORIGINAL, -I ERTL_IMPROVED, default/-m ERTL_MLE). */
#define DSH_ESTIM_ORIGINAL 0
#define DSH_ESTIM_ERTL_IMPROVED 1
#define DSH_ESTIM_ERTL_MLE 2

/* bns::EmissionType values, src/enums.h:13-23.  Symmetric measures handled by result_cmp's
 * first switch arm, src/dashing.h:571-576. */
#define DSH_MASH_DIST 0
#define DSH_JI 1
#define DSH_FULL_MASH_DIST 3
/* second arm of result_cmp (src/dashing.h:577-588), built on set_triple = full_set_comparison */
#define DSH_SIZES 2
#define DSH_FULL_CONTAINMENT_DIST 4
#define DSH_CONTAINMENT_INDEX 5
#define DSH_CONTAINMENT_DIST 6
#define DSH_SYMMETRIC_CONTAINMENT_INDEX 7
#define DSH_SYMMETRIC_CONTAINMENT_DIST 8

typedef struct dsh_ctx dsh_ctx;

/* ABI version: bumped whenever an entry point changes its signature or a table its layout (6: dsh_exchange_* take a
 * row-set table instead of bounds + world; 7: dsh_sketch_records*).  A host compiled against another DSH_ABI_VERSION links fine but would pass
 * shifted arguments: compare with dsh_abi_version() once at start-up.  (A bounds array handed to a function that now
 * parses a row-set table is refused, not over-read: its first word, 0, is not a valid world.)
 * Entry points that were only ADDED since leave the number alone and are detected by symbol (dlsym):
 * dsh_dist_threshold, dsh_dist_threshold_device, dsh_dist_rect_threshold, dsh_dist_pairs*, dsh_fold*,
 * dsh_upload_sketches_folded*, dsh_union_groups*, dsh_cluster_threshold, dsh_cluster_threshold_device, dsh_cluster_pairs,
 * dsh_cluster_csr, dsh_greedy_threshold, dsh_greedy_threshold_device, dsh_greedy_extend, dsh_greedy_extend_device,
 * dsh_group_stats, dsh_group_stats_device, dsh_dist_histogram, dsh_dist_histogram_device, dsh_dist_rect_histogram,
 * dsh_linkage_threshold, dsh_linkage_threshold_device, dsh_linkage_tri, dsh_mst, dsh_mst_tri, dsh_mst_linkage,
 * dsh_dbscan_threshold, dsh_dbscan_threshold_device, dsh_dbscan_tri, dsh_degree_threshold, dsh_degree_threshold_device,
 * dsh_union_curve, dsh_union_curve_device, dsh_curve_permutations, dsh_sketch_fastx_records. */
#define DSH_ABI_VERSION 7
int dsh_abi_version(void);

/* ---- context ---------------------------------------------------------------------------- */
const char *dsh_backend_name(void);       /* "hip:gfx950" */
int dsh_device_count(void);               /* number of visible HIP devices (0 if none) */
int dsh_create(int device, dsh_ctx **out);
void dsh_destroy(dsh_ctx *ctx);            /* waits for everything the context has enqueued before it releases anything */
const char *dsh_last_error(const dsh_ctx *ctx);
/* Load the kernels' code objects NOW (the HIP runtime otherwise loads each when one of its kernels is first launched:
 * 10-40 ms in the middle of the first sketch batch / the first dist call).  No context needed and safe to call from any
 * thread, also beside a thread that uses a context: a host that has something else to do while the runtime comes up (the
 * CLI stages its first batch) calls it there.  what: DSH_PRELOAD_SKETCH | DSH_PRELOAD_COMPARE. */
#define DSH_PRELOAD_SKETCH 1u
#define DSH_PRELOAD_COMPARE 2u
int dsh_preload(int device, unsigned what);
int dsh_synchronize(dsh_ctx *ctx);

/* ---- the resident sketch matrix ----------------------------------------------------------
 * Replaces `std::vector<hll_t> sketches` (src/sketch_and_cmp.h:282-288): n register arrays
 * of 2^p bytes, resident in HBM for the lifetime of the ctx (or until re-allocated).
 * p in [4,24] for sketching, cardinalities, up- and download (24 = the `hll` subcommand's default,
 * src/hllmain.cpp:5); the compare entry points take the same range (tuned for p <= 17; 20..24 work but are not a performance target). */
int dsh_sketches_alloc(dsh_ctx *ctx, uint64_t n, int p);
/* sketch.read(path) path (src/sketch_and_cmp.h:318-324, --presketched): host rows -> slots. */
int dsh_upload_sketches(dsh_ctx *ctx, const uint8_t *regs, uint64_t first_slot, uint64_t n);
int dsh_download_sketches(dsh_ctx *ctx, uint64_t first_slot, uint64_t n, uint8_t *regs_out);
/* Same, into a caller-owned DEVICE buffer (device-to-device on the ctx stream; returns when done).
 * Multi-GPU sketching: each rank sketches its share of the genomes, copies its rows
 * out with this call and the ranks all-gather the register arrays over RCCL. */
int dsh_copy_sketches_device(dsh_ctx *ctx, uint64_t first_slot, uint64_t n, void *d_regs_out);
/* Use a caller-owned DEVICE buffer [n][2^p] as the sketch matrix (no copy; the caller keeps it
 * alive).  This is how bench.py hands over inputs already resident in HBM. */
int dsh_attach_device_sketches(dsh_ctx *ctx, const void *d_regs, uint64_t n, int p);

/* ---- sketch waist -------------------------------------------------------------------------
 * Replaces the body of hot loop 1, `enc.for_each([&](u64 kmer){h.addh(kmer);}, file, ksp)`
 * (src/sketch_and_cmp.h:342 and :515; register rule mirrored at src/readfilt.cpp:86-88), for a
 * batch of genomes.  `seq` is host ASCII: genome g occupies seq[genome_off[g] .. genome_off[g+1]);
 * FASTA records inside a genome are separated by at least one non-ACGT byte (so k-mers never
 * span records, like kseq records); case is folded; any non-ACGT byte resets the window.
 * Canonical k-mers iff canon != 0 (-C clears it, src/distmain.cpp:65).  k in [1,32].
 * Registers go to slots [first_slot, first_slot+n_genomes) of the resident matrix (max-merged
 * into what is there, so a genome may be fed in several calls) and, if regs_out != NULL, are
 * also copied to the host.  Bit-exact with the CPU definition (max is order-independent).
 * Errors of every sketch entry point, returned before anything is enqueued: DSH_EINVAL for offsets
 * that decrease, a k outside [1,32], slots out of range or beyond 2^32 (the work lists keep a slot
 * in 32 bits); DSH_ESTATE before dsh_sketches_alloc. */
int dsh_sketch_batch(dsh_ctx *ctx, const uint8_t *seq, const uint64_t *genome_off,
                     uint32_t n_genomes, uint64_t first_slot, int k, int canon,
                     uint8_t *regs_out);
/* Asynchronous form: enqueues the host-to-device copy of `seq` (page-locked memory from dsh_alloc_host, else
 * the copy is synchronous) and the kernel, and returns; dsh_wait(ctx) completes it.  `seq` must stay untouched
 * until then.  A host that streams many genomes parses batch b+1 while batch b is copied and sketched. */
int dsh_sketch_batch_async(dsh_ctx *ctx, const uint8_t *seq_pinned, const uint64_t *genome_off,
                           uint32_t n_genomes, uint64_t first_slot, int k, int canon);
/* Same with `seq` already on the device (d_seq device pointer; genome_off stays on the host). */
int dsh_sketch_batch_device(dsh_ctx *ctx, const void *d_seq, const uint64_t *genome_off,
                            uint32_t n_genomes, uint64_t first_slot, int k, int canon);
/* Per-record sketches (upstream's sketch_by_seq / dist_by_seq, src/sketch_and_cmp.h:540-602): one sketch per RECORD.
 * Record r is seq[rec_off[r] .. rec_off[r+1]), the records lie back to back with NO separator between them, and its
 * registers go to slot first_slot + r.  k-mers never span two records, even where the bases on both sides of a boundary
 * are valid; inside a record the rules of dsh_sketch_batch hold (case folded, a non-ACGT byte resets the window).
 * Unlike dsh_sketch_batch the rows are OVERWRITTEN, not max-merged: afterwards row first_slot + r holds exactly the
 * registers of record r alone, and a record shorter than k has an all-zero row.  Slots outside
 * [first_slot, first_slot + n_records) are not touched.  k in [1,32], any p of dsh_sketches_alloc.
 * Errors, returned before anything is enqueued: DSH_EINVAL for a rec_off that decreases, a k outside [1,32] or slots out
 * of range; DSH_ESTATE before dsh_sketches_alloc.  The three forms take `seq` and their lifetimes exactly as the
 * dsh_sketch_batch trio does (host, page-locked host + dsh_wait, device: 32-byte aligned and padded by 128 bytes, rec_off
 * relative to d_seq and on the host). */
int dsh_sketch_records(dsh_ctx *ctx, const uint8_t *seq, const uint64_t *rec_off, uint32_t n_records, uint64_t first_slot,
                       int k, int canon, uint8_t *regs_out);
int dsh_sketch_records_async(dsh_ctx *ctx, const uint8_t *seq_pinned, const uint64_t *rec_off, uint32_t n_records,
                             uint64_t first_slot, int k, int canon);
int dsh_sketch_records_device(dsh_ctx *ctx, const void *d_seq, const uint64_t *rec_off, uint32_t n_records,
                              uint64_t first_slot, int k, int canon);
/* The same with the PARSE on the device, as in the reference where Encoder::for_each(func, path) reads the records itself
 * (src/sketch_and_cmp.h:338-342): `raw` holds the bytes of plain FASTA files as they lie on disk -- genome g's at
 * raw[genome_off[g] .. genome_off[g] + raw_len[g]) (several files of one genome: back to back with a '\n' between them),
 * its region [genome_off[g], genome_off[g+1]) at least that long, every genome_off[g] a multiple of 32.  The library
 * copies the raw bytes to the device and decodes them there into what kseq would hand the encoder, then sketches as
 * dsh_sketch_batch_async does (kseq: current klib's kseq_read).  A genome that begins with '>' is FASTA: header lines ('>'
 * or '@' first) end a record (one invalid byte: k-mers never span records), '\n' vanishes, a '\r' vanishes when a '\n'
 * follows it or it is the genome's last byte (kseq drops one '\r' that ends a line) and is otherwise an invalid byte,
 * everything else is sequence (validated and case-folded by the sketch kernel as above).  A genome that begins with '@' is
 * FASTQ in four-line records: of every four lines the second is sequence.  What does not keep its format's promise is
 * REFUSED per genome, never guessed at -- a FASTQ file with a '\r' that does not vanish or that begins a line, a first byte
 * that is neither, a FASTA line that begins with '+', a FASTQ file whose lines 4r are not '@' headers or 4r + 2 not '+'
 * lines, in which a sequence line begins with '@', '>' or '+', or in which some record's quality line is not exactly as
 * long as its sequence line (multi-line records, cut-off files: the record state of kseq decides those; the length rule
 * is checked as a 64-bit fingerprint over all records) -- : status_out[g] != 0, NOTHING goes into its slot, and the host
 * parses that genome itself
 * (dsh_sketch_batch) as kseq does: up to kseq's first error in a file, whose record contributes nothing.  status_out: n_genomes words of page-locked host memory (or NULL), valid after dsh_wait.  `raw` must
 * stay untouched until then.  Compressed inputs and pipes are the host's business (inflate, then either entry point). */
int dsh_sketch_fastx_batch_async(dsh_ctx *ctx, const uint8_t *raw_pinned, const uint64_t *genome_off,
                                 const uint64_t *raw_len, uint32_t n_genomes, uint64_t first_slot, int k, int canon,
                                 uint32_t *status_out_pinned);
/* Per-record sketches from raw file bytes: the device decodes the files as dsh_sketch_fastx_batch_async does and keeps, next
 * to the base stream, an index of where every record begins; then every record of every accepted file gets a row of its
 * own, OVERWRITTEN as by dsh_sketch_records.  Blocking.  `raw`, file_off[n_files + 1] and raw_len[n_files] are those of
 * dsh_sketch_fastx_batch_async (regions start on multiples of 32 and hold their file's raw bytes); one unit is ONE file,
 * and any host memory is taken (page-locked memory copies faster).
 *   slot_ptr[n_files + 1], monotone: file f owns the slots [slot_ptr[f], slot_ptr[f + 1]); its record r, in file order,
 *     goes to row slot_ptr[f] + r.
 *   status_out[n_files]: nonzero where the file is refused -- by the rules of dsh_sketch_fastx_batch_async, the early ones
 *     and the late one (the FASTQ length fingerprint).  A refused file writes no row and no hdr_off_out entry and reports
 *     n_rec_out[f] = 0: the caller parses it itself and uses dsh_sketch_records for its span.
 *   n_rec_out[n_files]: the records kseq reads from an accepted file (a header character that is the file's last byte
 *     starts none; a FASTQ file that ends inside a header line of two bytes or more ends with one more, empty record).
 *   hdr_off_out[slot_ptr[n_files] - slot_ptr[0]] or NULL: entry (slot - slot_ptr[0]) is the offset in `raw` of the record's
 *     '>' / '@'.  The record's name are the bytes behind it up to the first isspace byte or the file's end.
 * Count-only mode, slot_ptr == NULL: only the two scanning passes run; status_out (the EARLY refusals only: a file that
 * the full call refuses late is still counted here) and n_rec_out are filled, nothing is sketched; allowed before
 * dsh_sketches_alloc -- this is how a caller sizes its matrix.
 * If an accepted file's count differs from its span: DSH_ERANGE with a message in dsh_last_error, n_rec_out complete, NO
 * row of any file written (the convention of dsh_dist_threshold_device: call again with room).
 * Refused before anything is enqueued: DSH_EINVAL for k outside [1,32], a region that does not start on a multiple of 32 or
 * does not hold its raw_len, a slot_ptr that decreases, slots out of range; DSH_ESTATE before dsh_sketches_alloc (unless
 * count-only). */
int dsh_sketch_fastx_records(dsh_ctx *ctx, const uint8_t *raw, const uint64_t *file_off, const uint64_t *raw_len,
                             uint32_t n_files, const uint64_t *slot_ptr, int k, int canon, uint32_t *status_out,
                             uint64_t *n_rec_out, uint64_t *hdr_off_out);
int dsh_clear_sketches(dsh_ctx *ctx, uint64_t first_slot, uint64_t n);

/* ---- cardinalities ------------------------------------------------------------------------
 * Replaces cardinality_estimate(hll_t&) = h.report() (src/dashing.h:492, used at
 * src/sketch_and_cmp.h:377-382): one double per sketch. */
int dsh_cardinalities(dsh_ctx *ctx, int estim, double *card_out);

/* ---- compare waist ------------------------------------------------------------------------
 * Replaces hot loop 2: perform_core_op (src/sketch_and_cmp.h:699-710) / the oracle(i,j) of
 * dm::parallel_fill (distmat/distmat.h:459-512) with func = result_cmp (src/dashing.h:568-592):
 * for rows i in [row_begin,row_end) and all j>i, out[index(i,j) - index(row_begin,row_begin+1)]
 * = float(result_cmp(sketch_j, sketch_i, result_type, 1/k)).  The rows of a range are one
 * contiguous span of the packed triangle, dsh_tri_span() elements long.
 * result_type: any bns::EmissionType above; k only matters for the *_DIST forms.  In every pair the
 * reference calls result_cmp(lhs = sketch_j, rhs = sketch_i). */
int dsh_dist_rows(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t row_begin,
                  uint64_t row_end, float *out);
/* Same, result left in a caller-owned DEVICE buffer (no D2H).  The work runs on the ctx stream
 * (dsh_stream); the call returns after it has completed. */
int dsh_dist_rows_device(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t row_begin,
                         uint64_t row_end, void *d_out);
/* Asynchronous forms -- the reference overlaps the comparison of one batch of rows with the emission of
 * the previous one through two ping-pong buffers (dist_loop's dps[i & 1] + std::async writer,
 * src/sketch_and_cmp.h:804-816; parallel_fill's writer thread, distmat/distmat.h:475-479,504-508).  These
 * calls ENQUEUE the whole computation on the ctx stream and return.  For the host form the result goes to one of
 * two device buffers taken in turn and is copied to `out` on a second (copy) stream, so the kernels of the next call
 * run while the previous result is still travelling to the host; a call only waits for the copy that last drained
 * the buffer it is about to fill.  Calls may be issued back to back (their kernels execute in order).
 * Completion: dsh_wait(ctx) blocks until everything enqueued on the ctx (both streams) has completed;
 * dsh_event_record / dsh_event_wait mark and await one point of the sequence without draining what was enqueued
 * after it.  `out` must stay valid until then and should come from dsh_alloc_host: the copy into pageable memory is
 * staged by the runtime and is not asynchronous.
 * Typical use (the CLI does this):  async(block 0); t0 = record;  loop b: async(block b+1 -> buf[(b+1)&1]);
 * t(b+1) = record; event_wait(t(b)); emit block b from buf[b&1].
 * The call itself may still block briefly at its start while a new column layout is built on the host
 * (only the first call after the sketches changed touches the device for that). */
int dsh_dist_rows_async(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t row_begin,
                        uint64_t row_end, float *out_pinned);
int dsh_dist_rows_device_async(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t row_begin,
                               uint64_t row_end, void *d_out);
int dsh_wait(dsh_ctx *ctx);
/* Per-call completion.  dsh_event_record: *ticket marks everything enqueued on the ctx so far (kernels, sketch
 * batches, and the host copies of dsh_dist_rows_async).  dsh_event_wait blocks the calling host thread until that
 * point has completed; work enqueued after the record keeps running.  dsh_event_query: *done = 1/0 without blocking.
 * Tickets are cheap (a ring of 64 event pairs; a ticket more than 64 records old counts as complete).  A ticket is one
 * event on each of the context's two streams and orders NOTHING between them: taken between a compute call and
 * dsh_collect_parts_async it does not hold the per-part transfers back behind the kernels. */
int dsh_event_record(dsh_ctx *ctx, uint64_t *ticket);
int dsh_event_wait(dsh_ctx *ctx, uint64_t ticket);
int dsh_event_query(dsh_ctx *ctx, uint64_t ticket, int *done);
/* Make all work enqueued on the ctx stream AFTER this call wait for `hip_event` (a hipEvent_t recorded by
 * the caller on its own stream, e.g. torch.cuda.Event.cuda_event after producing d_regs / a gathered
 * staging buffer) -- the device-side alternative to synchronising the host before a *_device call. */
int dsh_wait_event(dsh_ctx *ctx, void *hip_event);
/* Row ranges and layouts: for a range of at least "range_sort_min_rows" rows (option, default 1024; always
 * for the full triangle) the plane matrix is rebuilt for exactly that range -- the wanted rows first, then the
 * later rows, both in (threshold, min value) order, earlier rows left out -- so every tile is homogeneous
 * (few planes) and every value is written at its final packed position: any split of the rows into
 * ranges concatenates to the byte-identical matrix, at the speed of the full-triangle call.  Smaller
 * ranges use the identity layout, which stays cached between calls. */
/* Query x reference rectangle (partdist_loop, src/dashing.h:660-712): queries are slots
 * [q_begin,q_end), references slots [r_begin,r_end); out[(qi-q_begin)*(r_end-r_begin)+(rj-r_begin)]. */
int dsh_dist_rect(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t q_begin,
                  uint64_t q_end, uint64_t r_begin, uint64_t r_end, float *out);

/* ---- k nearest neighbours -------------------------------------------------------------------
 * Replaces perform_nns / nndist_loop (src/sketch_and_cmp.h:642-783, --nearest-neighbors): for
 * every query slot in [q_begin,q_end) the nn best reference slots in [r_begin,r_end) under
 * result_type -- similarity measures best = largest, distances best = smallest (emt2nntype,
 * src/dashing.h:268-280) -- best first; a query is never its own neighbour.  Ties are broken by the
 * lower slot index (the reference's heap/thread order is unspecified).  idx_out/val_out: host
 * arrays [q_end-q_begin][nn]; missing neighbours (nn larger than the candidates) get idx 0xFFFFFFFF.
 * All-vs-all (nq == 0 in dashing): q = r = [0,n) -- every pair is computed ONCE.  Up to "knn_square_budget_bytes"
 * (option, default 96 GiB) both orientations go into an n x n float matrix in HBM and one selection pass per row
 * follows; beyond it (configs[4]: n x n would be 360 GB) the triangle is computed in bands of tile rows, every band
 * leaves its values as candidates of both sketches of each pair and is folded into the n running lists, so nothing of
 * size n x n exists (300 000 x p=14, nn=10: 14.7 s on one MI355X, one triangle pass).  nn > 1024 or q != r: blocks of
 * queries x all references. */
int dsh_knn(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t q_begin, uint64_t q_end,
            uint64_t r_begin, uint64_t r_end, uint32_t nn, uint32_t *idx_out, float *val_out);

/* ---- thresholded output: sparse hits instead of the dense matrix --------------------------------
 * Replaces what a dereplication or clustering client does with the output of dist_loop / partdist_loop
 * (src/sketch_and_cmp.h:785-830, src/dashing.h:660-712): scan the whole matrix for the pairs with, say, Jaccard >= t and
 * drop the rest.  Here the selection runs on the device, band by band (bands of whole rows of at most
 * "threshold_band_bytes" of float32, option, default 1 GiB), and only the hits leave it, as CSR:
 *   row_ptr  [rows + 1] uint64, relative to the first row of the call (row_ptr[0] = 0, row_ptr[rows] = n_hits)
 *   col      [n_hits] uint32, original slot numbers, ascending inside a row
 *   val      [n_hits] float32
 * The values are exactly the float32 values dsh_dist_rows / dsh_dist_rect give for the same estim, result_type and k
 * (that path computes them); a value passes by a float32 comparison with `threshold`: v >= threshold for the similarity
 * forms (JI, SIZES, CONTAINMENT_INDEX, SYMMETRIC_CONTAINMENT_INDEX), v <= threshold for the *_DIST forms (dsh_knn's
 * rule, emt2nntype, src/dashing.h:268-280); NaN never passes.  The same call on the same sketches gives the same bytes,
 * whatever the band size.  The calls are synchronous and leave the context free for any other call.
 * Triangle form: rows i in [row_begin,row_end) (row_end is cut at n; rows = what is left), columns j > i, in the ONE
 * orientation dsh_dist_rows computes, result_cmp(lhs = sketch_j, rhs = sketch_i): for the asymmetric measures
 * (CONTAINMENT_INDEX, CONTAINMENT_DIST, FULL_CONTAINMENT_DIST) the pair (i,j) is tested in that orientation only.
 * An empty range, n < 2, a threshold nothing passes and one everything passes are all valid.
 *   dsh_dist_threshold         host result.  row_ptr_out is the caller's [rows + 1]; *col_out / *val_out are allocated by
 *                              the library as dsh_alloc_host allocates (the number of hits is not known before the pass,
 *                              and counting first would pay the compare twice) and are released by the caller with
 *                              dsh_free_host, also when there is no hit.  col_out = val_out = NULL: counts only.
 *   dsh_dist_threshold_device  caller-owned DEVICE buffers: d_row_ptr [rows + 1] uint64, d_col / d_val of `cap` entries
 *                              (both NULL: counts only).  row_ptr and *n_hits are always complete; with *n_hits > cap
 *                              the first cap hits are written, nothing beyond, and the call returns DSH_ERANGE with a
 *                              message in dsh_last_error: call again with room for *n_hits.
 *   dsh_dist_rect_threshold    queries [q_begin,q_end) x references [r_begin,r_end) as dsh_dist_rect, one row per query,
 *                              col = reference slot; host result with the conventions of dsh_dist_threshold. */
int dsh_dist_threshold(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t row_begin, uint64_t row_end, float threshold,
                       uint64_t *row_ptr_out, uint32_t **col_out, float **val_out, uint64_t *n_hits);
int dsh_dist_threshold_device(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t row_begin, uint64_t row_end,
                              float threshold, void *d_row_ptr, void *d_col, void *d_val, uint64_t cap, uint64_t *n_hits);
int dsh_dist_rect_threshold(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t q_begin, uint64_t q_end, uint64_t r_begin,
                            uint64_t r_end, float threshold, uint64_t *row_ptr_out, uint32_t **col_out, float **val_out,
                            uint64_t *n_hits);

/* ---- an explicit list of pairs ------------------------------------------------------------------
 * Replaces result_cmp (src/dashing.h:568-592) called pair by pair: what a client does with the hits of
 * dsh_dist_threshold*, the lists of dsh_knn or the edges of a graph it keeps when it wants THOSE pairs again -- under
 * another measure, in the other orientation, with the set sizes -- without a second dense pass:
 *   out[t * n_pairs + x] = float(result_cmp(lhs = sketch[lhs[x]], rhs = sketch[rhs[x]], result_types[t], 1/k)),
 * 1/k being the float of dist_loop (src/sketch_and_cmp.h:797).  One read of the two register rows serves all n_types
 * measures (n_types <= 9).  The pairs are computed in the DIRECT form -- the exact histogram of max(a, b), then the
 * same estimator code as the dense path -- so:
 *   Values.  For every pair and every measure the float32 is bit for bit the one dsh_dist_rows writes at
 *     dsh_tri_index(n, i, j) when lhs = j > rhs = i, and the one dsh_dist_rect writes at [query = rhs][reference = lhs]
 *     for any two slots.  (dsh_knn's values use the double 1/k of nndist_loop, :729: they are not these.)
 *   Any pair is legal: lhs < rhs, lhs == rhs (the sketch with itself: what the formulas give, J = 1 for a non-empty
 *     sketch), repeated pairs, any order.  Output x belongs to input x.
 *   n_pairs == 0 and n_types == 0 succeed and write nothing.  DSH_EINVAL before anything is enqueued for a slot >= n (host
 *     and CSR forms; the device form checks on the device and fails the call after it, `out` then being unspecified), a
 *     result_type outside 0..8, n_types > 9, a row_ptr that decreases or a col out of range; DSH_ESTATE without sketches.
 *   Out-of-range registers (a value above 64 - p + 1): if a sketch NAMED BY A PAIR holds one the call fails with the
 *     dense path's code (DSH_EINVAL) and a message that names the sketch, `out` unspecified; sketches no pair names are
 *     not judged.
 *   The context's derived state is not touched: a pairs call between two dense calls changes neither's bytes, and
 *     costs neither a layout.  The cardinalities this path keeps (all n sketches, computed by the first call after the
 *     sketches or the estimator changed) are its own.
 *   Synchronous, on the ctx stream; the device form waits for the device once, at its end.  The list is worked off in
 *     chunks of "pairs_chunk" pairs (option, default 2^18; no result depends on it): scratch is 128 bytes (p <= 15;
 *     256 above) per pair of one chunk, whatever n_pairs is.
 *   Cost: 2 * 2^p bytes read per pair, against the dense path's fixed cost for all pairs.  Measured on one MI355X
 *     (profiles/pairs1/bench_pairs.jsonl): 179 M pairs/s at 10 000 x p=14, 1.3 G pairs/s at 100 000 x p=10;
 *     at 0.1 % of all pairs 41x and 77x faster than dsh_dist_rows_device of the full triangle.  Below about 5 % (p = 14)
 *     or 8 % (p = 10) of all pairs, ask for the pairs; above, compute the triangle.
 *   dsh_dist_pairs          lhs, rhs, out in host memory
 *   dsh_dist_pairs_device   d_lhs, d_rhs (uint32 [n_pairs]) and d_out (float32 [n_types][n_pairs]) in DEVICE memory; the
 *                           lists must be complete when the call is made (the ctx stream waits for no other stream)
 *   dsh_dist_pairs_csr      the pairs of a CSR result as dsh_dist_threshold* / dsh_dist_rect_threshold write it: hit h of
 *                           row r (row_ptr[r] <= h < row_ptr[r + 1]) is the pair (lhs = col[h], rhs = row_begin + r) --
 *                           the orientation both dense paths compute.  n_hits = row_ptr[rows] - row_ptr[0];
 *                           out[t * n_hits + (h - row_ptr[0])].  Under the measure that selected the hits this returns
 *                           their `val`. */
int dsh_dist_pairs(dsh_ctx *ctx, int estim, const int *result_types, uint32_t n_types, int k, const uint32_t *lhs,
                   const uint32_t *rhs, uint64_t n_pairs, float *out);
int dsh_dist_pairs_device(dsh_ctx *ctx, int estim, const int *result_types, uint32_t n_types, int k, const void *d_lhs,
                          const void *d_rhs, uint64_t n_pairs, void *d_out);
int dsh_dist_pairs_csr(dsh_ctx *ctx, int estim, const int *result_types, uint32_t n_types, int k, uint64_t row_begin,
                       uint64_t rows, const uint64_t *row_ptr, const uint32_t *col, float *out);

/* ---- derived sketches: fold to a lower p, union by groups ------------------------------------------
 * Replaces hll_t::compress (fold to a lower precision) and hll_t::operator+= (register-wise maximum) of the reference's
 * sketch library, as src/dashing.cpp:570-590 and src/union.cpp:33-58 use them one file at a time on the host: here they
 * make NEW sketch rows out of resident ones on the device, so that a matrix sketched once at a high p is compared at a
 * cheaper one, and a collection is collapsed into pan-sketches, without a trip over PCIe.  The result of a *_device form
 * is a plain [rows][2^p] matrix that dsh_attach_device_sketches takes as it is (16-byte aligned for that).
 *   Fold.  d = p - new_p; register j of a folded row is the maximum over the source registers idx in [j << d, (j+1) << d)
 *     of: 0 for an empty register, v + d where low = idx & (2^d - 1) is 0, else clz_d(low) + 1 (leading zeros of low in
 *     its d-bit field) -- what sketching the same input at new_p would have given.  new_p == p is a copy.
 *   Union.  out[g] = byte-wise max of the resident rows members[group_ptr[g] .. group_ptr[g+1]); an empty group gives an
 *     all-zero row; a slot may repeat inside a group and appear in several.  group_ptr [n_groups + 1] uint64 and members
 *     uint32 are HOST arrays in both forms (the call copies them to the device).
 *   Execution.  Synchronous, on the ctx stream; the *_device forms wait for the device once, at their end.
 *   Host forms.  Rows travel through bounded scratch: chunks of at most "derive_chunk_bytes" of source rows (option,
 *     default 256 MiB, at least one row; no result depends on it), so a call of any size works.  Page-locked memory from
 *     dsh_alloc_host makes the copies DMA; any host pointer works.  (dsh_union_groups stages its whole result.)
 *   No derived state touched.  dsh_fold* and dsh_union_groups* write only the caller's buffer (any alignment) and touch
 *     none of the context's derived state: a dense call before and after gives the same bytes and builds no new layout.
 *   dsh_upload_sketches_folded* writes slots [first_slot, first_slot + n) of a matrix from dsh_sketches_alloc
 *     (overwritten, other slots untouched) and invalidates exactly as dsh_upload_sketches does; with src_p == p it equals
 *     dsh_upload_sketches byte for byte.  d_regs: [n][2^src_p], any alignment (16-byte aligned is the fast path).
 *   Validation.  Fold and the folded upload fail with DSH_EINVAL and a message that names the sketch (slot number) when a
 *     source register exceeds 64 - src_p + 1, found on the device while the rows stream by; the output is then
 *     unspecified.  Union does not judge registers.
 *   Argument errors, before anything is enqueued: DSH_EINVAL for slots out of range, new_p outside [4, p], src_p outside
 *     [p, 24], a group_ptr that decreases or a member >= n; DSH_ESTATE without sketches (the folded upload: without
 *     dsh_sketches_alloc).  n == 0 and n_groups == 0 succeed and write nothing.
 *   Cost.  Pure streaming: fold moves 1 + 2^-d bytes per source byte, union 1 + groups/members; a device-to-device copy
 *     of the same source moves 2.  Not yet measured on the device (tools/bench_derive.py does it). */
/* rows [first_slot, first_slot+n) of the resident matrix folded to new_p (4 <= new_p <= p): out [n][2^new_p] */
int dsh_fold(dsh_ctx *ctx, uint64_t first_slot, uint64_t n, int new_p, uint8_t *regs_out);
int dsh_fold_device(dsh_ctx *ctx, uint64_t first_slot, uint64_t n, int new_p, void *d_out);
/* rows at src_p >= the context's p, folded on the device INTO slots [first_slot, first_slot+n) (overwritten) */
int dsh_upload_sketches_folded(dsh_ctx *ctx, const uint8_t *regs, int src_p, uint64_t first_slot, uint64_t n);
int dsh_upload_sketches_folded_device(dsh_ctx *ctx, const void *d_regs, int src_p, uint64_t first_slot, uint64_t n);
/* out[g] = max over members[group_ptr[g] .. group_ptr[g+1]) of the resident rows; group_ptr, members on the HOST */
int dsh_union_groups(dsh_ctx *ctx, const uint64_t *group_ptr, const uint32_t *members, uint64_t n_groups, uint8_t *regs_out);
int dsh_union_groups_device(dsh_ctx *ctx, const uint64_t *group_ptr, const uint32_t *members, uint64_t n_groups, void *d_out);

/* ---- union growth curves: how the union grows along an order of resident sketches ---------------------
 * The k-mer pangenome growth (collector's) curve: the cardinality of the union of the first i + 1 sketches of an order,
 * for every i, and over many orders (permutations) its mean and spread.  The registers of that union are the running
 * byte-wise maximum along the order and the cardinality is the estimator on that row's histogram, so the curve is exact
 * for the HLLs that are resident; a register moves about ln(len) times, so the per-prefix histograms are the prefix sums
 * of a sparse stream of "moved from bin a to bin b at step i" events and every order reads every row ONCE.
 *   Orders.  orders is row-major uint32 [n_orders][len]; every entry is a slot < n.  Repeats are legal: a repeated slot
 *     changes nothing.  HOST memory in dsh_union_curve, DEVICE memory in dsh_union_curve_device.
 *   Outputs.  card_out[o * len + i] (float64) is the `estim` estimate (DSH_ESTIM_ORIGINAL, _ERTL_IMPROVED, _ERTL_MLE) of the
 *     union of the sketches orders[o][0 .. i], computed by the estimator kernel of dsh_dist_pairs from the prefix's
 *     histogram: two prefixes with equal histograms carry bit-identical doubles.  hist_out / d_hist may be NULL; otherwise
 *     it is uint32 [n_orders][len][DSH_CURVE_BINS]: bin v = the number of registers of that union holding v; every prefix's
 *     histogram sums to 2^p.  Exactly n_orders * len doubles and n_orders * len * 64 uint32 are written, nothing else.
 *     d_card is 8-byte, d_hist 4-byte aligned device memory.
 *   len == 0 or n_orders == 0 returns DSH_OK, writes nothing and launches nothing.
 *   Errors.  DSH_EINVAL: a NULL context, a bad estim, a NULL orders / card pointer; an entry >= n (the message names the
 *     order and the position); a NAMED sketch that holds a register above 64 - p + 1 (the message names the smallest such
 *     slot, in the words of dsh_dist_pairs) -- a sketch no order names is not judged.  DSH_ESTATE without resident
 *     sketches.  DSH_ENOMEM, with a message, when scratch cannot be allocated: never a partial result.  The entries are
 *     validated on the host before any launch (the device form copies them back for that: 4 bytes per step).  On an error
 *     dsh_union_curve leaves card_out / hist_out untouched; dsh_union_curve_device leaves unspecified contents but never
 *     writes outside the caller's spans.
 *   State.  Reads the resident rows, owned or attached; neither reads nor invalidates the compare path's derived state
 *     (a dense call before and after gives the same bytes).  A dsh_upload_sketches between two calls is seen by the second.
 *   Execution.  Synchronous, on the ctx stream; one wait for the device at the end.  Orders run in batches whose deltas
 *     (256 bytes per step), counters (128, above p = 15 256) and segment start rows stay within "curve_scratch_bytes"
 *     (option, default 256 MiB; one order alone that needs more grows the scratch to that).  A long order is cut into
 *     segments of "curve_segment" members (option; 0 = the planner's choice, about 2048 workgroups per launch and no
 *     segment below 64 members) whose unions come from the kernel of dsh_union_groups, so that one order fills the
 *     device.  No result depends on either option.  The host form also holds the orders (4 bytes per step), the
 *     cardinalities (8) and one batch's histograms on the device, and with several batches the histograms in host memory
 *     of its own until the call is known to succeed.
 *   Cost model: (1 or 2) x n_orders x len x 2^p bytes of rows (2 with segments), plus n_orders x len x 256
 *     bytes of deltas written and read once.  Measured on one MI355X (tools/bench_curve.py, profiles/curve1): 10 000 x p=14
 *     one order 0.28 ms, 100 permutations 6.1 ms (device copies of the same rows: 7.3 ms); 100 000 x p=10 one order 0.74 ms,
 *     20 permutations 4.0 ms (the copies: 0.82 ms; at p = 10 the deltas and counters are 37 % of the row bytes again).
 *   dsh_curve_permutations writes n_perm permutations of 0 .. n - 1 as uint32 [n_perm][n]; pure host, a pure function of
 *     (n, seed, r).  Permutation r runs splitmix64 from the state x = seed + r (wrapping); next() is x += 0x9E3779B97F4A7C15,
 *     z = x, z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9, z = (z ^ z >> 27) * 0x94D049BB133111EB, return z ^ z >> 31.  The shuffle is
 *     Fisher-Yates from the identity: for i = n - 1 down to 1, swap [i] and [next() % (i + 1)].  n >= 2^32 and a NULL out
 *     with n * n_perm > 0 give DSH_EINVAL.
 *   Not built: a multi-GPU form, orders over a second context's rows, --groups in the CLI (curves per group), and the
 *     greedy "largest gain next" order. */
#define DSH_CURVE_BINS 64
int dsh_union_curve(dsh_ctx *ctx, int estim, const uint32_t *orders, uint64_t len, uint64_t n_orders,
                    double *card_out, uint32_t *hist_out);
int dsh_union_curve_device(dsh_ctx *ctx, int estim, const void *d_orders, uint64_t len, uint64_t n_orders,
                           void *d_card, void *d_hist);
int dsh_curve_permutations(uint64_t n, uint64_t n_perm, uint64_t seed, uint32_t *out);   /* pure host */

/* ---- clusters at a threshold: connected components on the device --------------------------------------
 * Replaces what a dereplication or clustering client does with the hits of dsh_dist_threshold*: build the graph whose
 * edges are the passing pairs and read off its connected components (single linkage) with a union-find on the host.  At
 * 100 000 sketches a loose threshold gives 10^8 to 10^9 hits -- gigabytes of col / val that exist only to be united; here
 * they are united where they are computed and `n` labels leave the device.
 *   The result.  Let G be the graph on the slots 0..n-1 whose edges are exactly the hits of
 *     dsh_dist_threshold(ctx, estim, result_type, k, 0, n, threshold, ...): the same float32 values, the same predicate
 *     (v >= threshold for the similarity forms, v <= threshold for the *_DIST forms, NaN never) and, for the asymmetric
 *     measures, the ONE orientation of the triangle.  labels[x] is the smallest slot of the connected component of x;
 *     *n_clusters is the number of x with labels[x] == x.  This has one answer: it depends on no band size, launch
 *     geometry or order of arrival of atomics, and the same call gives the same bytes.
 *   How.  A union-find over parent[n] in device memory with parent[x] <= x at all times; its only writes are the hook
 *     (compare-and-swap of a root under a SMALLER root) and path shortening (atomic minimum with an ancestor), so the
 *     root a component ends with is its smallest member and no renumbering pass exists.  Every loop of the kernels counts
 *     its steps against n + 1; an overrun -- unreachable while the invariant holds -- fails the call with DSH_EIO and the
 *     message "internal: union-find step bound exceeded" instead of hanging the device.
 *   dsh_cluster_threshold         labels_out: host uint32 [n].  Bands of whole rows as dsh_dist_threshold ("threshold_band_bytes",
 *                                 at most 2^20 rows), computed by the dense path into a library-owned buffer and walked once;
 *                                 no hit is written, no host wait between bands, one wait at the end.  The effects on the
 *                                 context's cached state are exactly those of dsh_dist_threshold on rows [0, n): the dense
 *                                 calls before and after give the same bytes.
 *   dsh_cluster_threshold_device  d_labels: caller-owned DEVICE uint32 [n]; exactly n labels are written.
 *   dsh_cluster_pairs             the components of a caller's graph on n_nodes nodes (n_nodes is the caller's choice: no
 *                                 sketches are needed, only the stream and scratch): edges (lhs[x], rhs[x]) in host memory, in
 *                                 any order, self loops and repeated edges legal.  labels_in NULL, or [n_nodes]: an earlier
 *                                 labelling to continue from (x starts united with labels_in[x]) -- how the hits of several
 *                                 row ranges, ranks or calls are merged: pass the labels_out of one call to the next.
 *   dsh_cluster_csr               the same for a CSR as dsh_dist_threshold* / dsh_dist_rect_threshold write it: hit h of row r
 *                                 (row_ptr[r] <= h < row_ptr[r + 1]) is the edge (row_begin + r, col[h]).
 *   The edge list is worked off in chunks of "cluster_chunk" edges (option, default 2^20; no result depends on it): device
 *     scratch is 8 bytes per edge of one chunk (CSR: 4, and 8 per row) whatever the length of the list.
 *   Errors, before anything is enqueued: DSH_EINVAL for a node, col or labels_in entry >= n_nodes, a row_ptr that decreases,
 *     rows outside [0, n_nodes) and n_nodes (or n) > 2^32 - 1; DSH_ESTATE for the threshold forms without sketches.
 *     n == 0, n < 2, n_pairs == 0 and rows == 0 succeed; a NaN threshold gives n singletons.
 *   Synchronous, on the ctx stream.  Cost model: the dense path's cost for the triangle plus ONE read of
 *     each band (4 bytes per pair) and two small reads of parent[] per hit; dsh_dist_threshold_device + dsh_cluster_csr
 *     reads each band twice and writes 8 bytes per hit.  Not yet measured on the device (tools/bench_cluster.py does it).
 *   Not built: a multi-GPU form (merge per-rank labels with dsh_cluster_pairs' labels_in) and clusters of a rectangle.
 *     Complete and average linkage: dsh_linkage_* below. */
int dsh_cluster_threshold(dsh_ctx *ctx, int estim, int result_type, int k, float threshold, uint32_t *labels_out,
                          uint64_t *n_clusters);
int dsh_cluster_threshold_device(dsh_ctx *ctx, int estim, int result_type, int k, float threshold, void *d_labels,
                                 uint64_t *n_clusters);
int dsh_cluster_pairs(dsh_ctx *ctx, uint64_t n_nodes, const uint32_t *lhs, const uint32_t *rhs, uint64_t n_pairs,
                      const uint32_t *labels_in, uint32_t *labels_out, uint64_t *n_clusters);
int dsh_cluster_csr(dsh_ctx *ctx, uint64_t n_nodes, uint64_t row_begin, uint64_t rows, const uint64_t *row_ptr, const uint32_t *col,
                    const uint32_t *labels_in, uint32_t *labels_out, uint64_t *n_clusters);

/* ---- single-, complete- and average-linkage clusters at a threshold --------------------------------------
 * Replaces what a clustering client (dRep's primary step, ANI / Mash pipelines) does when it cuts an average- or
 * complete-linkage tree at a threshold: pull the dense matrix to the host and run a host `linkage` on it.  Here the
 * agglomeration runs on the device, component by component, and `n` labels leave it.
 *   Values.  v(x, y), x != y, is the float32 that dsh_dist_rows leaves at dsh_tri_index(n, min, max): the ONE orientation
 *     of the triangle (dsh_linkage_tri: the caller's tri[dsh_tri_index(n, min, max)]).  desc = the measure is a similarity
 *     (better = larger; the *_DIST forms: better = smaller; dsh_linkage_tri: the caller's `descending`).  Floats compare as
 *     integer keys of the same order compare them: -0.0 equals +0.0, +-inf are ordinary values, NaN is special (below).
 *     q(v) = llrint((double)v * 2^DSH_STATS_FRAC_BITS), exactly as dsh_group_stats defines it.
 *   Clusters.  A cluster is a set of slots, its label its smallest slot; at the start every slot is a cluster.  For two
 *     clusters A != B the pair is either BLOCKED or has a value D(A, B):
 *       DSH_LINKAGE_SINGLE    the best v over the member pairs that are not NaN; blocked iff all of them are NaN
 *       DSH_LINKAGE_COMPLETE  the worst v over the member pairs; blocked iff any is NaN
 *       DSH_LINKAGE_AVERAGE   the exact rational S / c, S = the sum of q(v) over the member pairs (int64), c = |A| |B|;
 *                             blocked iff any member pair is NaN or has |v| >= 2 (the rule dsh_group_stats includes a pair by)
 *     D passes the threshold t iff, SINGLE and COMPLETE: the float predicate of dsh_dist_threshold (>= for similarities, <=
 *     for distances, NaN never); AVERAGE: S >= Q c (similarity) or S <= Q c (distance) with Q = q(t), compared exactly in
 *     128-bit integers.  AVERAGE therefore judges QUANTISED values: a value within 2^-31 of t may be judged equal to t.
 *   The procedure (the definition, not the implementation).  While some unblocked pair of current clusters passes, take the
 *     one with the best D -- AVERAGE: the rationals compared exactly by cross-multiplication -- ties to the
 *     lexicographically smallest (label(A), label(B)) with label(A) < label(B); replace A and B by their union.
 *     labels[x] is the label of x's final cluster, *n_clusters the number of x with labels[x] == x.  This has one answer:
 *     it depends on no band size, route, partition, launch geometry or order of arrival, and the same call gives the same
 *     bytes.
 *   Consequences.  SINGLE equals dsh_cluster_threshold byte for byte (it exists as the check of the machinery: it agglomerates
 *     every component pair by pair, so call dsh_cluster_threshold for single linkage).  Every COMPLETE or AVERAGE cluster lies
 *     inside one SINGLE cluster at the same t (AVERAGE: at the loose threshold below).  In a COMPLETE cluster every member's
 *     `worst` of dsh_group_stats passes t.  The Lance-Williams updates are exact in this arithmetic: the best or worst of two
 *     keys, S(A u B, C) = S(A, C) + S(B, C), and blocked is absorbing for COMPLETE and AVERAGE.
 *   How.  Every merge needs a passing member pair, so the connected components of the graph of passing pairs
 *     split the problem: they come from the union-find of dsh_cluster_threshold at t -- for AVERAGE at the loose float
 *     threshold t' whose graph is the quantised one (distance: the largest float32 with q(t') <= Q; similarity: the smallest
 *     with q(t') >= Q).  Components of one slot are done.  Each of the others gets an m x m matrix of cells (uint32 keys;
 *     int64 sums for AVERAGE) in device scratch and ONE workgroup (k_linkage), which agglomerates it to the end with a
 *     nearest-neighbour entry per row; components run side by side in batches whose matrices fit "linkage_budget_bytes"
 *     (default 8 GiB).  The matrices are filled by one of two routes, as in dsh_group_stats: dense (the band walk again, a
 *     kernel that stores the pairs inside a component) or pairs (the intra-component pairs enumerated on the device and
 *     computed by the direct pair path).  Option "linkage_route": -1 auto | 0 dense | 1 pairs; auto takes pairs iff
 *     20 P_in <= n (n - 1) / 2, P_in the pairs inside components; dsh_get_info(ctx, "linkage_route") is the route the last
 *     dsh_linkage_threshold* call took.  With several batches the dense route walks the triangle once per batch.
 *     "linkage_partition" 0 treats the whole collection as one component; "linkage_lds_max" (default 4096, at most 6144) is
 *     the largest component whose per-row state lives in LDS rather than in global scratch.  No result depends on an option.
 *     Every loop of the kernel counts against the component's size + 1; an overrun -- unreachable in a correct kernel --
 *     fails the call with DSH_EIO and the message "internal: linkage step bound exceeded".
 *   dsh_linkage_threshold         labels_out: host uint32 [n].
 *   dsh_linkage_threshold_device  d_labels: caller-owned DEVICE uint32 [n]; exactly n labels are written.
 *   dsh_linkage_tri               the same for a caller's values (ANI, say): tri holds n_nodes (n_nodes - 1) / 2 float32 in host
 *                                 memory in dsh_tri_index order; no sketches are needed, only the stream and scratch.  The
 *                                 triangle travels through the band buffer ("threshold_band_bytes") band by band, once for the
 *                                 components and once per batch.
 *   Synchronous, on the ctx stream; the only host wait beyond the final one is the one the component labels need.  The effects
 *     on cached state are those of dsh_cluster_threshold, plus those of dsh_dist_pairs_device on the pairs route: a dense call
 *     before and a dense call after give the same bytes.
 *   Errors, before anything is enqueued: as dsh_cluster_threshold (DSH_ESTATE without sketches, n > 2^32 - 1); DSH_EINVAL for
 *     an unknown linkage, AVERAGE with DSH_SIZES, AVERAGE with |threshold| >= 2, n_nodes > 2^32 - 1 and a NULL tri with
 *     n_nodes >= 2.  After the component labels: DSH_ENOMEM, with a message that names m and the bytes, for one component whose
 *     matrix exceeds "linkage_budget_bytes" (or, AVERAGE, of more than 65536 members: its sums are 64-bit); the context stays
 *     usable.  A NaN threshold gives n singletons; n == 0 and n == 1 succeed.
 *   Not built: the merge list (a dendrogram) of complete or average linkage (the single-linkage dendrogram is dsh_mst below), a
 *     component larger than one workgroup's budget spread over several workgroups,
 *     Ward / centroid linkages, a multi-GPU form.  Cost: about 1-2 ms per merge step of a component of ~3000 members on an MI355X
 *     (DESIGN.md 4.15); tools/bench_linkage.py is the benchmark, which has not been run to its end. */
#define DSH_LINKAGE_SINGLE 0
#define DSH_LINKAGE_COMPLETE 1
#define DSH_LINKAGE_AVERAGE 2
int dsh_linkage_threshold(dsh_ctx *ctx, int estim, int result_type, int k, float threshold, int linkage, uint32_t *labels_out,
                          uint64_t *n_clusters);
int dsh_linkage_threshold_device(dsh_ctx *ctx, int estim, int result_type, int k, float threshold, int linkage, void *d_labels,
                                 uint64_t *n_clusters);
int dsh_linkage_tri(dsh_ctx *ctx, uint64_t n_nodes, const float *tri, int descending, float threshold, int linkage,
                    uint32_t *labels_out, uint64_t *n_clusters);

/* ---- minimum spanning tree of the pair values: the single-linkage dendrogram, on the device ------------------
 * Replaces what a client does today for the single-linkage tree (a guide tree, or the clusters at EVERY threshold): pull the
 * n (n - 1) / 2 matrix to the host and run a host `linkage` on it, or call dsh_cluster_threshold once per candidate threshold.
 * The single-linkage dendrogram is the minimum spanning tree of the pair values: n - 1 edges.
 *   Values: for slots x != y, v(x, y) is the float32 dsh_dist_rows leaves at dsh_tri_index(n, min, max) -- the ONE orientation of
 *     the triangle, as in dsh_cluster_threshold (dsh_mst_tri: the caller's tri[dsh_tri_index(n, min, max)]).  desc = the measure
 *     is a similarity (better = larger; the *_DIST forms: better = smaller; dsh_mst_tri: the caller's `descending`).  Values
 *     compare as floats do with -0.0 equal to +0.0; +-inf are ordinary values.
 *   The graph G: the pair {x, y} is an edge iff v is not NaN and passes `cutoff` by the float predicate of dsh_dist_threshold
 *     (v >= cutoff for similarities, v <= cutoff for distances).  A NaN cutoff passes nothing (dsh_cluster_threshold's rule); for
 *     "no cutoff" pass -INFINITY (similarity) or +INFINITY (distance).
 *   Edge order: the edge (i, j), i < j, is better than another iff it comes first lexicographically by (the better value, the
 *     smaller i, the smaller j).  This is a strict total order, so G has exactly ONE best spanning forest: the one Kruskal's
 *     algorithm builds when it takes the edges in this order.  It is the result.
 *   Output: *n_edges = n - (components of G); lhs_out[e] < rhs_out[e] (uint32) and val_out[e] (float32: the pair's dense value,
 *     a zero as +0.0), sorted best first in the order above; the caller sizes the three arrays for n - 1 entries.  labels_out
 *     (host uint32 [n], or NULL): the smallest slot of x's component of G, byte for byte what dsh_cluster_threshold gives at
 *     `cutoff`.  The result depends on no band size, launch geometry or order of arrival of atomics: the same call gives the
 *     same bytes.
 *   Consequence: for any t at least as tight as `cutoff`, the edges whose value passes t are a prefix of the list, and
 *     dsh_cluster_pairs over that prefix equals dsh_cluster_threshold at t byte for byte -- one call stands in for a cluster call
 *     at every threshold.
 *   dsh_mst          over the resident sketches.
 *   dsh_mst_tri      the same for a caller's values (ANI, say): tri holds n_nodes (n_nodes - 1) / 2 float32 in host memory in
 *                    dsh_tri_index order; no sketches are needed, only the stream and scratch.
 *   dsh_mst_linkage  pure host, no context: the sorted edge list as a merge table in scipy's Z convention.  Leaves are
 *                    0 .. n - 1; step s joins the current clusters of lhs[s] and rhs[s] into cluster n + s; za[s] < zb[s] are the
 *                    two cluster ids, zv[s] = val[s], zsize[s] the member count.  A forest of fewer than n - 1 edges is legal and
 *                    gives n_edges rows.  DSH_EINVAL if an edge names a node >= n_nodes or joins two nodes that are already
 *                    united (the list is not a forest), or a NULL array with n_edges > 0.
 *   How: Boruvka rounds over the band walk of dsh_cluster_threshold ("threshold_band_bytes").  Per round the component labels of
 *     the union-find, one pass of k_mst_band over every band -- a passing value between two components offers (value, partner)
 *     to both ends under a 64-bit maximum --, per component the best offer of its members, and the chosen edges appended and
 *     united; one 8-byte read of the edge count is the round's only host wait.  The components with an outgoing edge at least
 *     halve per round, so at most floor(log2 n) + 1 rounds emit; dsh_get_info(ctx, "mst_rounds") is the number of the last call.
 *     The loop is bounded at 34 rounds: an overrun is unreachable in a correct build and fails the call with DSH_EIO and the
 *     message "internal: mst round bound exceeded".  The edges (12 bytes each) come to the host once and are sorted there.
 *   Cost: rounds x one dense pass.  Where the whole triangle is ONE band (10 000 sketches at the default 1 GiB) it is computed,
 *     or uploaded, once and walked again by every round; else every round recomputes (dsh_mst) or uploads again (dsh_mst_tri)
 *     its bands.  Per pair and round the walk reads up to 16 bytes (value, label, best offer) where k_cc_band reads 4
 *     (tools/bench_mst.py is the benchmark: on an MI355X 15.0 ms at 10 000 x p=14, where one cluster call takes
 *     14.0, and 2.07 s at 100 000 x p=10, seven dense passes).  Scratch: 32 bytes per slot beside the cluster call's.
 *   Synchronous, on the ctx stream.  The effects on cached state are exactly those of dsh_cluster_threshold: a dense call before
 *     and a dense call after give the same bytes.
 *   Errors, before anything is enqueued, as dsh_cluster_threshold / dsh_linkage_tri: DSH_ESTATE without sketches (dsh_mst);
 *     DSH_EINVAL for n > 2^32 - 1, for a NULL lhs_out, rhs_out, val_out or n_edges with n >= 2, and for a NULL tri with
 *     n_nodes >= 2.  n == 0 and n == 1 succeed with 0 edges.
 *   Not built: a device-resident output form (the result is at most 12 (n - 1) bytes and is sorted on the host), a rectangle, a
 *     multi-GPU form, merge lists for complete or average linkage. */
int dsh_mst(dsh_ctx *ctx, int estim, int result_type, int k, float cutoff, uint32_t *lhs_out, uint32_t *rhs_out, float *val_out,
            uint64_t *n_edges, uint32_t *labels_out);
int dsh_mst_tri(dsh_ctx *ctx, uint64_t n_nodes, const float *tri, int descending, float cutoff, uint32_t *lhs_out, uint32_t *rhs_out,
                float *val_out, uint64_t *n_edges, uint32_t *labels_out);
int dsh_mst_linkage(uint64_t n_nodes, const uint32_t *lhs, const uint32_t *rhs, const float *val, uint64_t n_edges, uint32_t *za,
                    uint32_t *zb, float *zv, uint32_t *zsize);

/* ---- density clusters at a threshold (DBSCAN) and the degrees of the threshold graph, on the device ---------
 * Single linkage (dsh_cluster_threshold) chains: at a loose threshold one bridge input welds two groups into one component.
 * DBSCAN keeps the components' cost and cuts the bridges: only inputs with enough neighbours carry a cluster.  What a client
 * does today is bring the CSR of dsh_dist_threshold to the host (10^8 to 10^9 hits at 100 000 sketches) to count neighbours.
 *   The graph G on the slots 0 .. n - 1: its edges are exactly the hits of dsh_dist_threshold(ctx, estim, result_type, k, 0, n,
 *     threshold, ...) -- the same float32 values, the same predicate (v >= threshold for the similarity forms, v <= threshold for
 *     the *_DIST forms, NaN never) and, for the asymmetric measures, the ONE orientation of the triangle, as in
 *     dsh_cluster_threshold (dsh_dbscan_tri: the caller's tri[dsh_tri_index(n, min, max)] and `descending`).
 *   degree[x] (uint32): the edges at x, whether x is their row or their column.
 *   x is a CORE iff degree[x] + 1 >= min_pts, compared in 64 bits: the point counts itself, as in the DBSCAN paper and in
 *     scikit-learn.  min_pts is at least 1.
 *   Clusters: the connected components of G restricted to the edges between two cores; the label of a cluster is its smallest
 *     core slot.
 *   A non-core x with at least one core neighbour is a BORDER and takes the label of ONE core neighbour c:
 *       DSH_GREEDY_FIRST: the smallest such c;
 *       DSH_GREEDY_BEST:  the c with the best value v(c, x); values that are equal as float32 (-0.0 equal to +0.0) go to the
 *                         smaller c.
 *     A border is never a bridge: nothing is united through it.  Every other non-core is NOISE and labelled with itself.
 *   Output: labels[x] (uint32) as above, with labels[labels[x]] == labels[x].  NOTE that a border's label may be LARGER than
 *     its own slot (the label is the cluster's smallest CORE): the labels are group ids as dsh_group_stats accepts them, not
 *     "the smallest member".  kind[x] (uint8, optional): DSH_DBSCAN_NOISE, DSH_DBSCAN_BORDER or DSH_DBSCAN_CORE.  degree[x]
 *     (uint32, optional).  *n_clusters = the cores with labels[x] == x; *n_noise (optional) = the noise points.  A NULL optional
 *     output is not written.  The result depends on no band size, launch geometry or order of arrival of atomics.
 *   Consequences.  min_pts == 1: every slot is a core and labels, n_clusters equal dsh_cluster_threshold's byte for byte.
 *     min_pts == 2: the labels still equal them (the singletons are noise, labelled with themselves) and n_clusters is the
 *     components' count minus n_noise.  min_pts > n: everything is noise.  A non-core has at most min_pts - 2 edges.
 *   dsh_dbscan_threshold          over the resident sketches; host outputs, [n] each.
 *   dsh_dbscan_threshold_device   the three arrays are caller-owned DEVICE buffers; exactly n items of each are written.
 *   dsh_dbscan_tri                the same for a caller's values (ANI, say): tri holds n_nodes (n_nodes - 1) / 2 float32 in host
 *                                 memory in dsh_tri_index order; no sketches are needed, only the stream and scratch.
 *   dsh_degree_threshold(_device) the degrees alone: how many inputs lie within the threshold of each input.
 *   How: two walks over the band walk of dsh_cluster_threshold ("threshold_band_bytes").  Walk 1 counts the degrees with a number
 *     of atomics that does not grow with the hits (one per 4096-value chunk of a row and one per column and slab of 512 rows that
 *     saw a hit).  Walk 2 unites the two ends of a passing value in the union-find of dsh_cluster_threshold where both are
 *     cores, and where exactly one is, offers it to the other end under a 64-bit maximum (value key, then the smaller core); a
 *     non-core has at most min_pts - 2 edges, so these offers are bounded by n (min_pts - 2) whatever the threshold.  One more
 *     launch writes labels, kinds and counts.  No hit is written, no host wait between bands, one wait at the end.
 *   Cost: where the whole triangle is ONE band (10 000 sketches at the default 1 GiB) its values stay on the device between the
 *     walks: one dense pass and two reads of the span.  Else walk 2 recomputes (dsh_dbscan_tri: uploads again) its bands and the
 *     call costs about two dense passes; dsh_degree_threshold* always costs one.  Scratch: 13 bytes per slot beside the cluster
 *     call's.  tools/bench_dbscan.py is the benchmark.
 *   Synchronous, on the ctx stream.  The effects on cached state are exactly those of dsh_dist_threshold: a dense call before
 *     and a dense call after give the same bytes.
 *   Errors, before anything is enqueued, as dsh_cluster_threshold / dsh_greedy_extend: DSH_ESTATE without sketches (not
 *     dsh_dbscan_tri); DSH_EINVAL for n > 2^32 - 1, for min_pts == 0, for an unknown assign_mode, for a NULL labels (or degrees, for
 *     dsh_degree_threshold*) output with n > 0, and for a NULL tri with n_nodes >= 2.  n == 0 succeeds with zero counts.
 *   Not built: a CSR / edge-list form, a rectangle, a multi-GPU form, a weighted degree, OPTICS / HDBSCAN, and keeping the hits
 *     as a bit mask between the walks instead of recomputing the bands of a triangle of several bands. */
#define DSH_DBSCAN_NOISE 0
#define DSH_DBSCAN_BORDER 1
#define DSH_DBSCAN_CORE 2
int dsh_dbscan_threshold(dsh_ctx *ctx, int estim, int result_type, int k, float threshold, uint32_t min_pts, int assign_mode,
                         uint32_t *labels_out, uint8_t *kind_out, uint32_t *degree_out, uint64_t *n_clusters, uint64_t *n_noise);
int dsh_dbscan_threshold_device(dsh_ctx *ctx, int estim, int result_type, int k, float threshold, uint32_t min_pts, int assign_mode,
                                void *d_labels, void *d_kind, void *d_degree, uint64_t *n_clusters, uint64_t *n_noise);
int dsh_dbscan_tri(dsh_ctx *ctx, uint64_t n_nodes, const float *tri, int descending, float threshold, uint32_t min_pts, int assign_mode,
                   uint32_t *labels_out, uint8_t *kind_out, uint32_t *degree_out, uint64_t *n_clusters, uint64_t *n_noise);
int dsh_degree_threshold(dsh_ctx *ctx, int estim, int result_type, int k, float threshold, uint32_t *degree_out);
int dsh_degree_threshold_device(dsh_ctx *ctx, int estim, int result_type, int k, float threshold, void *d_degree);

/* ---- greedy representatives at a threshold: the greedy pass in slot order, on the device ---------------
 * Replaces what a dereplication client does with the hits of dsh_dist_threshold* when it wants REPRESENTATIVES rather than
 * components (CD-HIT, dRep, galah): walk the inputs in priority order, make an input no earlier representative covers a
 * representative, and give every other input to its first representative -- a sequential pass on the host over 10^8 to
 * 10^9 hits at 100 000 sketches and a loose threshold.  Single linkage (dsh_cluster_threshold) does not answer this:
 * components chain, and the smallest slot of a component represents members it does not resemble at all.
 *   The result.  Let hit(i, j), i < j, be "the pair (i, j) is a hit of dsh_dist_threshold(ctx, estim, result_type, k, 0, n,
 *     threshold, ...)": the same float32 value, the same predicate (v >= threshold for the similarity forms, v <= threshold
 *     for the *_DIST forms, NaN never) and, for the asymmetric measures, the ONE orientation of the triangle.  Priority is
 *     slot order (the caller orders the slots).  The representative set R is defined by: x is in R iff there is no r in R
 *     with r < x and hit(r, x) -- the lexicographically first maximal independent set of the hit graph.  labels[x] = x
 *     for x in R; otherwise labels[x] is the SMALLEST r in R with r < x and hit(r, x).  *n_reps is the number of x with
 *     labels[x] == x.  Consequences: labels[x] <= x; labels[labels[x]] == labels[x]; every non-representative passes the
 *     threshold against its label; no two representatives pass against each other; and the labels of the slots [0, m) are
 *     those of a call on the first m sketches alone (prefix property): appending inputs never relabels earlier ones.  This
 *     has one answer: it depends on no band size, launch geometry or order of arrival of atomics.
 *   How.  One uint32 assign[n] in device memory, assign[x] = x at the start and only ever lowered; assign[x] < x means
 *     "covered by that representative".  Bands of whole rows in ascending order, as dsh_cluster_threshold computes them.
 *     Per band [b0, b1): k_greedy_diag -- ONE workgroup with assign[b0..b1) in LDS walks the band's rows in ascending order;
 *     a row that is still itself covers the passing in-band columns that are still themselves (each column belongs to one
 *     thread: no atomics; one barrier per representative row; the values are loaded 16 rows at a time, so that their
 *     latencies overlap; a row covered before its batch touches no memory) -- then k_greedy_band: every
 *     representative row of the band lowers assign[j] to itself (atomic minimum) for its passing columns j >= b1; a covered
 *     row's waves return at once.  k_greedy_labels writes the labels and counts after the last band.  No loop waits for
 *     another thread, so unlike the union-find of the clusters there is no step bound and no give-up path.
 *   dsh_greedy_threshold         labels_out: host uint32 [n].
 *   dsh_greedy_threshold_device  d_labels: caller-owned DEVICE uint32 [n]; exactly n labels are written.
 *   Execution.  Synchronous, on the ctx stream; no host wait between bands, one wait at the end.  The band rule is
 *     dsh_dist_threshold's ("threshold_band_bytes", at most 2^20 rows) with one more cap, "greedy_band_rows" rows (option,
 *     default 4096, 1..8192; no result depends on it): it bounds the LDS of k_greedy_diag at 32 KiB.  The effects on the
 *     context's cached state are exactly those of dsh_dist_threshold on rows [0, n): the dense calls before and after give
 *     the same bytes.
 *   Errors, before anything is enqueued: DSH_EINVAL for a NULL context, a NULL output with n > 0 and n > 2^32 - 1;
 *     DSH_ESTATE without sketches.  n == 0 and n < 2 succeed; a NaN threshold gives n representatives.
 *   Cost model: the dense path's cost for the triangle, ONE read of each band outside its diagonal block
 *     by the rows that are representatives (4 bytes per pair of those rows; a covered row costs nothing), one atomic per
 *     hit that lowers a label, and the sequential diagonal: per band, one barrier per representative row and one round of
 *     global loads per 16 rows, in ONE workgroup.  Its worst case is a threshold nothing passes (every row a
 *     representative).  Measured on one MI355X (tools/bench_greedy.py, profiles/greedy1; G = this call,
 *     C = dsh_cluster_threshold_device, A = the dense call): at 100 000 x p=10 (A = 288 ms) G - A = 10.0 / 9.1 / 7.5 ms at
 *     0.1 % / 1 % / 50 % hits beside C - A = 3.5 / 7.2 / 16.4 ms, and 94 ms where nothing passes (C - A = 3.5 ms), about
 *     four fifths of it k_greedy_diag; at 10 000 x p=14 (A = 14.1 ms) G - A = 5.5 / 4.6 / 1.5 ms and 7.7 ms where nothing
 *     passes, C - A within 1.3 ms of zero.  G - A is below A everywhere.
 *   Not built: a caller-given priority permutation (the caller orders the slots); a rectangle form; CSR or edge-list
 *     forms (a sequential host pass over hits that are already on the host is linear); a multi-GPU form.  Assignment to
 *     the BEST representative and a continuation behind an existing labelling are dsh_greedy_extend*, below. */
int dsh_greedy_threshold(dsh_ctx *ctx, int estim, int result_type, int k, float threshold, uint32_t *labels_out,
                         uint64_t *n_reps);
int dsh_greedy_threshold_device(dsh_ctx *ctx, int estim, int result_type, int k, float threshold, void *d_labels,
                                uint64_t *n_reps);

/* ---- greedy representatives, continued: extend a labelling, assign to the best representative --------------
 * What the users of CD-HIT, dRep and galah ask for next.  A collection grows: a release appends a few per cent of genomes
 * to a database that is already dereplicated, and by the prefix property above the old labels cannot change -- only the
 * pairs (old representative, new slot) and (new, new) matter: m (n - m) + (n - m)^2 / 2 pairs instead of n^2 / 2 for m old
 * slots, at most (no row of an old slot that is not a representative is computed where a whole band holds none).  And a
 * covered slot may go to the BEST representative that hits it rather than the first (CD-HIT -g 1).
 *   The result.  hit(i, j), i < j, and v(i, j), its value, are those of dsh_dist_threshold(ctx, estim, result_type, k, 0, n,
 *     threshold, ...): the same float32, the same predicate, the same single orientation.  m = first_new.
 *     Old slots: labels[x] = labels_in[x] for x < m; old slots are never re-judged, in either mode.
 *     R_old = {x < m : labels_in[x] == x} is taken as given: it need not be what a full call would have produced, so
 *     extending a set of representatives chosen elsewhere is legal and defined.
 *     New slots x >= m, in ascending order: x is in R iff no r in R_old or in R with m <= r < x has hit(r, x).  Otherwise
 *       DSH_GREEDY_FIRST: labels[x] is the smallest such r;
 *       DSH_GREEDY_BEST:  labels[x] is the such r with the best v(r, x) -- the largest for the similarity forms, the
 *         smallest for the *_DIST forms, compared as float32 (so -0.0 equals +0.0); ties go to the smallest r.
 *     *n_reps is the number of x in [0, n) with labels[x] == x.  This has one answer: it depends on no band size, launch
 *     geometry or order of arrival of atomics.
 *   Consequences.  first_new == 0 with DSH_GREEDY_FIRST equals dsh_greedy_threshold byte for byte.  If labels_in is the
 *     first m labels of a full call (first_new == 0) in the same mode, the result is that full call's result.
 *     first_new == n copies labels_in and counts.  BEST and FIRST have the same representatives.  In BEST every covered
 *     x >= m still passes against its label, and no other representative r < x has a strictly better value.
 *   How.  assign[n] as above, started from labels_in below m.  In BEST one uint64 best[n - m], 0 = none, raised with a plain
 *     64-bit atomic maximum: the high word is the value as an order-preserving integer (the two zeros made one,
 *     complemented for the *_DIST forms), the low word 0xFFFFFFFF - r.  Phase 1: bands of old rows from a representative
 *     to a representative (at most "threshold_band_bytes" of values and 2^20 rows; a stretch without one is skipped),
 *     computed as the rectangle [b0, b1) x [m, n) -- bit for bit the triangle's values, see dsh_dist_pairs above -- and
 *     walked by k_greedy_rect: a wave of a row that is no representative returns at once, a passing column is lowered in
 *     assign and, in BEST, raised in best.  Phase 2: the band loop of dsh_greedy_threshold started at row m with
 *     k_greedy_diag and k_greedy_band unchanged; in BEST k_greedy_best stands in k_greedy_band's place: the band's
 *     representative rows raise best for all their passing columns, in-band ones included, and lower assign for the
 *     later ones (one read of a band outside its diagonal block, the block a second time).  k_greedy_extend_labels
 *     writes the labels: assign[x], or in BEST for a covered new slot the slot its key names.
 *   dsh_greedy_extend         labels_out: host uint32 [n].
 *   dsh_greedy_extend_device  d_labels: caller-owned DEVICE uint32 [n]; exactly n labels are written.
 *   labels_in is a HOST array [first_new] in both forms, NULL if and only if first_new == 0.
 *   Execution.  Synchronous, on the ctx stream; no host wait between bands, one at the end.  The effects on the context's
 *     cached state are those of dsh_dist_rect_threshold on [0, m) x [m, n) followed by dsh_dist_threshold on rows [m, n):
 *     the dense calls before and after give the same bytes.
 *   Errors, before anything is enqueued: DSH_EINVAL for a NULL context, first_new > n, an assign_mode outside {0, 1},
 *     labels_in NULL with first_new > 0 (or not NULL with first_new == 0), an x with labels_in[x] > x or
 *     labels_in[labels_in[x]] != labels_in[x] (the message names x), a NULL output with n > 0 and n > 2^32 - 1; DSH_ESTATE
 *     without sketches.  n == 0 and n < 2 succeed; a NaN threshold makes every new slot a representative.
 *   Cost model: the dense path's cost for the old-representative bands of the rectangle and for the
 *     triangle rows [m, n), one read of each, and in BEST one more read of each diagonal block and one 64-bit atomic per
 *     hit of a representative row that raises a key.  Not yet measured on the device (tools/bench_greedy_extend.py does it).
 *   Not built: the old representatives gathered into a compact matrix first (the rows between two representatives of a
 *     band are computed and not read); a caller-given priority permutation; a rectangle / classify-only form (new slots
 *     against representatives, no new representatives); CSR or edge-list forms; a multi-GPU form; re-judging old slots
 *     when a new slot would have been a better representative. */
#define DSH_GREEDY_FIRST 0
#define DSH_GREEDY_BEST 1
int dsh_greedy_extend(dsh_ctx *ctx, int estim, int result_type, int k, float threshold, int assign_mode,
                      uint64_t first_new, const uint32_t *labels_in, uint32_t *labels_out, uint64_t *n_reps);
int dsh_greedy_extend_device(dsh_ctx *ctx, int estim, int result_type, int k, float threshold, int assign_mode,
                             uint64_t first_new, const uint32_t *labels_in, void *d_labels, uint64_t *n_reps);

/* ---- statistics of a labelling: per-group counts, sums, worst values and medoids, on the device -----------
 * What a client asks about the labels of dsh_cluster_*, dsh_greedy_* or its own group ids next: how far has a component
 * chained (its worst intra-group value), how well does each member sit in its group (its mean value to the others), and
 * which member should represent it (the medoid, not the smallest slot).  Without this call the answer needs the hits of
 * dsh_dist_threshold at a threshold loose enough to hold every intra-group pair, or the dense matrix, on the host.
 *   Labels.  labels is a HOST uint32 [n] in both forms; any values < n are legal; a group is the set of slots with equal
 *     labels.  Nothing else is required of them (labels[labels[x]] need not be labels[x]).
 *   v(x, y), x != y: the float32 dsh_dist_rows writes at dsh_tri_index(n, min(x, y), max(x, y)) -- for the asymmetric
 *     measures the ONE orientation of the triangle, as in the cluster and greedy calls.  A pair is INCLUDED iff v is not
 *     NaN and |v| < 2 (every measure but DSH_SIZES lives there for real sketches; DSH_SIZES is refused with DSH_EINVAL).
 *     q(v) = llrint((double)v * 2^DSH_STATS_FRAC_BITS), round to nearest even; the product is exact in double.
 *   cnt[x]    the number of y != x in x's group whose pair with x is included.
 *   sum[x]    the sum of q(v(x, y)) over those y, int64 (n <= 2^32 - 1 and |q| < 2^31 keep it inside); the mean value of x
 *             to its group is sum / cnt / 2^DSH_STATS_FRAC_BITS.
 *   worst[x]  the worst included value: the smallest for the similarity forms, the largest for the *_DIST forms, compared
 *             as float32 with -0.0 equal to +0.0 (a zero is reported as +0.0); NaN when cnt[x] == 0.  The diameter of a
 *             group is the worst worst[x] over its members.
 *   medoid[x] the member m of x's group chosen by three keys in turn: the largest cnt[m]; then the best sum[m] (largest
 *             for the similarity forms, smallest for the *_DIST forms); then the smallest slot.  A singleton is its own.
 *   Any output pointer may be NULL: that output is not written; exactly n entries of every other one are.
 *   This has one answer: all accumulation is in integers (32-bit counts, 64-bit sums, the worst value as an order-preserving
 *     32-bit key under an integer maximum; no float atomics), so it depends on no band size, route, launch geometry or order
 *     of arrival of atomics, and the same call gives the same bytes.
 *   Two routes, one result.  P_in = the intra-group pairs, sum over the groups of s (s - 1) / 2, known on the host.
 *     dense: the band loop of dsh_cluster_threshold ("threshold_band_bytes", at most 2^20 rows) with two kernels per band:
 *       k_gs_rows (one wave per 4096-value chunk of a row; at most one set of three atomics per wave, none where no column
 *       of the chunk is in the row's group) and k_gs_cols (a thread per column walks the band's rows above it in slabs of
 *       512 rows; at most one set per column and slab).  The number of atomics does not grow with the matching pairs.
 *     pairs: the member lists of the groups of two or more (4 bytes per slot, 12 per group) go to the device; k_gs_enum
 *       writes the intra-group pairs chunk by chunk ("pairs_chunk") as lhs = the larger slot, rhs = the smaller -- the
 *       orientation for which dsh_dist_pairs_device gives the triangle's bits -- the direct pair path computes them and
 *       k_gs_pairs folds each value into both ends.  Nothing of the size of P_in crosses PCIe or exists at once.
 *     Option "stats_route": -1 auto | 0 dense | 1 pairs; no result depends on it.  Auto takes the pairs route iff
 *       20 * P_in <= n (n - 1) / 2: the 5 % break-even of pair lists above, which the measurement of this call
 *       confirms (below).  dsh_get_info(ctx, "stats_route") is the route the last call took.
 *   Out-of-range registers: each route fails as its machinery does, DSH_EINVAL with a message that names the sketch, the
 *     outputs unspecified.  The dense route judges ALL sketches; the pairs route only those inside a group of two or more.
 *   Cached state.  After the dense route it is as after dsh_dist_threshold on rows [0, n), after the pairs route as after
 *     dsh_dist_pairs_device: a dense call before and after either gives the same bytes.
 *   Execution.  Synchronous, on the ctx stream; no host wait between bands or chunks, one at the end.
 *   Errors, before anything is enqueued: DSH_EINVAL for a NULL context, n > 2^32 - 1, a label >= n (the message names the
 *     slot), DSH_SIZES, an estimator or result_type out of range; DSH_ESTATE without sketches.  n == 0 and n == 1 succeed.
 *   Cost model: dense = the dense path's cost for the triangle plus two more reads of each band (values
 *     and labels for the rows, labels from LDS and the matching values for the columns: at most 8 bytes per pair);
 *     pairs = 2 * 2^p bytes per intra-group pair.  Measured on one MI355X (tools/bench_group_stats.py, profiles/stats1;
 *     A = the dense call): at 100 000 x p=10 (A = 282 ms) dense - A = 5.3 ms at P_in = 0.01 % of all pairs to 16.7 ms at
 *     100 %, pairs = 0.87 ms to 4.8 s; at 10 000 x p=14 (A = 13.0 ms) dense - A stays below 0.5 ms, pairs = 0.26 ms to 288 ms.
 *     The routes cost the same at P_in = 4.1 % (p = 14) and 5.7 % (p = 10) of all pairs.
 *   dsh_group_stats         the four outputs in host memory.
 *   dsh_group_stats_device  the four outputs caller-owned DEVICE arrays [n] (d_sum 8-byte aligned).
 *   Not built: a multi-GPU form; statistics of a rectangle; relabelling to medoids inside the cluster / greedy calls (the
 *     client maps labels -> medoid[labels]); weighted members. */
#define DSH_STATS_FRAC_BITS 30
int dsh_group_stats(dsh_ctx *ctx, int estim, int result_type, int k, const uint32_t *labels, uint32_t *medoid_out,
                    uint32_t *cnt_out, int64_t *sum_out, float *worst_out);
int dsh_group_stats_device(dsh_ctx *ctx, int estim, int result_type, int k, const uint32_t *labels, void *d_medoid,
                           void *d_cnt, void *d_sum, void *d_worst);

/* ---- value histograms of the triangle and of a rectangle: the distribution of the values, on the device -----
 * Every selection above is driven by one number the caller must already know: the threshold.  This call is how to choose
 * it: the values of a triangle or rectangle call are counted over up to DSH_HIST_MAX_EDGES caller-given bin edges in ONE
 * dense pass, optionally split into the intra-group and inter-group pairs of a labelling, and only the counts --
 * planes * (n_edges + 2) 64-bit integers -- leave the device.
 *   Values counted.  Triangle forms: exactly the float32 values dsh_dist_rows writes for rows [row_begin, row_end),
 *     columns j > i (row_end is cut at n); for the asymmetric measures the ONE orientation of the triangle.  Rectangle
 *     form: exactly the values dsh_dist_rect writes, self pairs included where the ranges overlap.  Any result_type the
 *     dense path takes.
 *   Edges.  edges is a HOST float32 [n_edges] in all forms, 1 <= n_edges <= DSH_HIST_MAX_EDGES, strictly increasing under
 *     float32 comparison, no NaN; -inf and +inf are legal; -0.0 followed by +0.0 is NOT increasing.
 *   Classes.  There are n_edges + 2 of them, and the closed side of an edge is the side that passes as a threshold:
 *     similarity forms: class(v) = the number of edges e with e <= v; the bins are [e_{b-1}, e_b)  (every measure that
 *                       is no *_DIST form, DSH_SIZES included: what dsh_dist_threshold passes with v >= t);
 *     *_DIST forms:     class(v) = the number of edges e with e <  v; the bins are (e_{b-1}, e_b];
 *     NaN is class n_edges + 1 (which nothing else reaches); -0.0 and +0.0 are one value.
 *     Consequence: for every b, the n_hits of dsh_dist_threshold over the same rows at threshold = edges[b] is, for the
 *     similarity forms, the sum of the classes b + 1 .. n_edges, and for the *_DIST forms the sum of the classes 0 .. b.
 *     One call therefore gives the exact hit counts at up to 4096 thresholds (e.g. the cap of dsh_dist_threshold_device).
 *     The sum of all classes is the number of pairs of the call.
 *   Labels.  labels is NULL, or a HOST uint32 [n] indexed by slot; any values are legal, only equality matters.
 *     NULL: counts is [1][n_edges + 2].  Not NULL: counts is [2][n_edges + 2]; plane 0 holds the pairs whose two slots carry
 *     equal labels (intra), plane 1 the others (inter).  In the rectangle the row is the query slot, the column the
 *     reference slot; a self pair is intra.
 *   Counts.  uint64, OVERWRITTEN (not added to); exactly planes * (n_edges + 2) entries are written.  d_counts is a
 *     caller-owned DEVICE buffer, 8-byte aligned.  All accumulation is in integers: the result depends on no band size,
 *     launch geometry or order of arrival of atomics, and the same call gives the same bytes.
 *   Execution.  Synchronous, on the ctx stream: the band loop of dsh_dist_threshold ("threshold_band_bytes", at most 2^20
 *     rows) with one launch of k_hist per band; no host wait between bands, one at the end.  k_hist keeps the edges and
 *     32-bit counters in LDS (sized from n_edges), runs as a bounded grid whose waves stride over the band's 4096-value
 *     chunks, finds a value's class by a binary search of at most 13 steps (none while a lane's values stay in one class),
 *     counts the lanes of a wave that share a class with ONE LDS add, and flushes its non-zero counters once per launch with
 *     64-bit atomic adds.  A workgroup's share of a band is kept below 2^32 values by the grid rule, whatever the band size.
 *   Cached state.  Exactly the effects of dsh_dist_threshold / dsh_dist_rect_threshold over the same rows: a dense call
 *     before and after gives the same bytes.
 *   Errors, before anything is enqueued: DSH_EINVAL for a NULL context, n_edges == 0 or > DSH_HIST_MAX_EDGES, NULL edges or
 *     a NULL output, edges not strictly increasing or NaN (the message names the index), rectangle slots beyond n, an
 *     estimator or result_type out of range; DSH_ESTATE without sketches.  An empty range (row_begin >= row_end after the
 *     cut, as the threshold forms judge it) or n < 2 succeeds with all-zero counts.  Out-of-range registers fail as the
 *     dense path does, the counts unspecified.
 *   Cost model: the dense path's cost for the same rows plus one read of each band, 4 bytes per pair, plus
 *     4 more with labels: about 5 ms at 100 000 x p=10.  Measured on one MI355X (tools/bench_hist.py, profiles/hist1;
 *     H = dsh_dist_histogram_device, A = dsh_dist_rows_device of the full triangle, MASH_DIST): at 100 000 x p=10
 *     (A = 281 ms) H - A = 4.6 ms at 2 edges and 4.9 ms at 101 edges where ONE class holds every value (5.8 / 5.7 ms with
 *     labels), 8.4 ms at 4096 (15 ms with labels); where half of the values are spread over the classes 12.6 ms at 2 edges,
 *     22 ms at 101 (23 ms with labels), 46 ms at 4096 (60 ms with labels).  The one-class case is the cheapest; with
 *     spread values the cost grows with the steps of the search, about 3 ms each.  At 20 000 x p=12 with continuous values
 *     (A = 45.6 ms) H - A = 0.2 ms in one class, 0.9 ms evenly spread over 101 edges, 1.6 ms over 4096.  At 10 000 x p=14
 *     (A = 12.7 ms) H - A is below 0.25 ms up to 101 edges, 0.4 ms (1.0 ms with labels) at 4096.
 *   dsh_dist_histogram         triangle rows, counts in host memory.
 *   dsh_dist_histogram_device  triangle rows, counts in the caller's device buffer.
 *   dsh_dist_rect_histogram    query slots [q_begin, q_end) x reference slots [r_begin, r_end), counts in host memory.
 *   Not built: a multi-GPU form (the caller adds the counts of row ranges); per-slot histograms; weighted members;
 *     quantiles computed by the library (the cumulative sums of the counts give them to the resolution of the edges). */
#define DSH_HIST_MAX_EDGES 4096
int dsh_dist_histogram(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t row_begin, uint64_t row_end,
                       const float *edges, uint32_t n_edges, const uint32_t *labels, uint64_t *counts_out);
int dsh_dist_histogram_device(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t row_begin, uint64_t row_end,
                              const float *edges, uint32_t n_edges, const uint32_t *labels, void *d_counts);
int dsh_dist_rect_histogram(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t q_begin, uint64_t q_end,
                            uint64_t r_begin, uint64_t r_end, const float *edges, uint32_t n_edges,
                            const uint32_t *labels, uint64_t *counts_out);

/* ---- multi-GPU shards of the full triangle ------------------------------------------------
 * Every rank holds all sketches (dsh_upload/attach) and computes one shard; no collective is
 * needed inside the compare.  Internally the plane matrix is laid out in (threshold, min value)
 * order so that tiles need few planes; shards are contiguous row ranges of THAT order, balanced
 * by cost, so a shard's result is one contiguous span of the packed triangle of the sorted order.
 *   dsh_shard_plan        span_off[0..nshards] = element offsets of the shards' spans (identical
 *                         on every rank: it depends only on the sketches)
 *   dsh_dist_shard_device compute shard `shard` into d_span (span_off[shard+1]-span_off[shard]
 *                         floats, device memory)
 *   dsh_unpermute_device  after the spans were gathered back to back (e.g. RCCL gather):
 *                         sorted-order packed triangle -> packed triangle in the original sketch
 *                         order (distmat/distmat.h:260-264), device to device. */
int dsh_shard_plan(dsh_ctx *ctx, int estim, uint32_t nshards, uint64_t *span_off);
int dsh_dist_shard_device(dsh_ctx *ctx, int estim, int result_type, int k, uint32_t shard,
                          uint32_t nshards, void *d_span);
int dsh_unpermute_device(dsh_ctx *ctx, const void *d_sorted_tri, void *d_out_tri);
/* Same, reading the spans where a gather of equal-sized (padded) blocks left them: shard r's span
 * starts at d_stage + r * stride (floats), stride >= the largest span.  Saves the copy that would lay
 * the spans back to back first.  Returns after completion. */
int dsh_unpermute_staged_device(dsh_ctx *ctx, const void *d_stage, uint64_t stride, uint32_t nshards,
                                void *d_out_tri);
/* General form: shard r's span starts at d_stage + block_off[r] (floats) -- any arrangement of the
 * gathered blocks, e.g. the per-piece blocks of a pipelined gather (several shards per rank, each
 * piece gathered while the next is computed). */
int dsh_unpermute_blocks_device(dsh_ctx *ctx, const void *d_stage, const uint64_t *block_off,
                                uint32_t nshards, void *d_out_tri);

/* ---- multi-GPU exchange over RCCL / xGMI ------------------------------------------------------
 * One dsh_ctx per GPU; the ranks may be processes (one per GPU, the bench) or threads of one process (the CLI).
 * The compare needs no collective -- every rank holds all sketches and computes a row range whose result is ONE
 * contiguous span of dashing's packed matrix (dsh_balance_rows) -- so the only exchange is the delivery of the spans
 * to the rank that emits the matrix, as in dashing where one process writes it (src/sketch_and_cmp.h:838-849), and,
 * when sketching is shared out, the all-gather of the register arrays.  RCCL is loaded on first use (librccl.so.1
 * next to the HIP runtime this library links to; DSH_RCCL_LIB overrides); all traffic is enqueued on the ctx stream,
 * so it is ordered with the kernels without any host synchronisation.
 *   dsh_comm_unique_id   rank 0: 128 bytes (an ncclUniqueId) to hand to every rank (file, pipe, MPI, shared memory ...)
 *   dsh_comm_init        collective (blocks until all `world` ranks called it with the same id)
 *   dsh_collect_spans    after rank r computed rows [bounds[r], bounds[r+1]) into d_local (device, its span): grouped
 *                        ncclSend/ncclRecv, one message per peer, every span received at its final place in d_final
 *                        (device, n(n-1)/2 floats, only read on `dst`; dst's own span is copied there unless d_local
 *                        already points at it).  The _async form returns after enqueueing (dsh_wait / a ticket).
 *   dsh_allgather_device ncclAllGather of equal-sized byte blocks (d_recv: world x bytes_per_rank), e.g. the register
 *                        arrays after sharded sketching (dsh_copy_sketches_device gives the block)
 *   dsh_dist_collect     the whole multi-GPU dist step for a host without device pointers: computes this rank's row
 *                        range, delivers the spans to `dst`, which gets the full packed matrix in `out` (host,
 *                        n(n-1)/2 floats; ignored on other ranks).  Without a communicator (world = 1) it is dsh_dist_rows.
 *                        bounds = NULL: the library partitions the rows itself (dsh_balance_rowsets) and runs the
 *                        pipelined exchange pair below.
 * Pipelined form (the exchange hidden behind the compute): dsh_dist_rows_parts_device_async computes a row range in
 * `nparts` consecutive parts (dsh_range_parts: about equal pair counts, cuts on whole 128-row tile rows; the plane
 * matrix keeps every part key-ordered on its own) and marks the completion of each part on the ctx stream;
 * dsh_collect_parts_async then enqueues, on the copy stream, one round of grouped ncclSend/ncclRecv per part, each
 * round waiting only for its own part -- part q travels over xGMI while part q+1 is computed.  Every rank calls both
 * with the same bounds / nparts; dsh_comm_wait (or dsh_wait / a ticket) completes them.  A range of any length works: a
 * call with parts always lays its range out in exactly the parts dsh_range_parts reports (a short range: one part),
 * and a rank without rows simply takes no part in the rounds.
 * ENVIRONMENT INPUTS of the library (all read by the exchange only):
 *   DSH_RCCL_LIB             path of the RCCL library to dlopen instead of librccl.so.1.  A CODE-LOADING TRUST BOUNDARY:
 *                            whatever it names runs inside the process that called dsh_comm_* (the tests load the
 *                            stand-in transport tests/mock_rccl through it).  A set-uid / privileged host must clear it.
 *                            If set and not loadable, dsh_comm_available reports DSH_ENODEV (never a silent fallback).
 *   DSH_COMM_INIT_TIMEOUT_S  seconds dsh_comm_init waits for ncclCommInitRank (default 90).  A timeout is FATAL for the
 *                            job: the helper thread stays inside RCCL, and should the peers arrive later the orphan
 *                            communicator is aborted, so that they fail too instead of waiting for this rank.
 *   DSH_COMM_TIMEOUT_S       seconds dsh_comm_wait and the blocking exchange calls wait (default 120)
 * Failure behaviour (a multi-rank job must end with an error, not hang):
 *   dsh_comm_available   DSH_OK if librccl can be loaded here (DSH_ENODEV otherwise) -- local, no communication: let
 *                        every rank check it and agree BEFORE the collective dsh_comm_init
 *   dsh_comm_library     the resolved path of the loaded librccl and its ncclGetVersion code (for logs)
 *   dsh_comm_init        gives up after DSH_COMM_INIT_TIMEOUT_S (default 90 s) when not every rank joins
 *   dsh_comm_wait        like dsh_wait, but with a deadline (DSH_COMM_TIMEOUT_S, default 120 s): when a peer never posts
 *                        its side of an exchange the communicator is aborted and DSH_EIO returned; the blocking
 *                        exchange calls (dsh_collect_spans, dsh_allgather_device, dsh_dist_collect) wait the same way */
#define DSH_UNIQUE_ID_BYTES 128
int dsh_range_parts(uint64_t n, uint64_t row_begin, uint64_t row_end, uint32_t nparts, uint64_t *part_rows, /* [nparts + 1] */
                    uint32_t *nparts_out);
int dsh_dist_rows_parts_device_async(dsh_ctx *ctx, int estim, int result_type, int k, uint64_t row_begin, uint64_t row_end,
                                     void *d_out, uint32_t nparts);
int dsh_collect_parts_async(dsh_ctx *ctx, uint64_t n, const uint64_t *bounds, uint32_t nparts, const void *d_local,
                            void *d_final, int dst);
/* The exchange-aware pair.  Parts of consecutive rows are key-ordered each on its own, so a SHORT range cut into many
 * parts loses the ordering its tiles live on (one 128-row block per part: 10 planes per tile instead of 8.7 at BASELINE
 * configs[2] over 8 ranks), and contiguous ranges on 128-row boundaries cannot give every rank the same number of tiles
 * when a range is only a few tile rows long (tile rows hold 79 ... 1 tiles there, a rank ~395).  So the partition is a
 * ROW-SET TABLE -- row segments with owners:
 *     tab[0] = world, tab[1] = nseg, tab[2 .. 2 + nseg] = the nseg + 1 segment boundaries from 0 to n,
 *     tab[3 + nseg .. 3 + 2 nseg) = the owning rank of every segment                       (3 + 2 nseg words)
 * A rank's rows are the segments it owns (adjacent ones merged): the first is its MAIN range, the others EXTRA segments
 * ("top-ups"); a rank with extra segments must have all its boundaries on multiples of 128 (or at n).
 *   dsh_balance_rowsets      main ranges over the top of the triangle + the short tile rows at its bottom dealt, in runs
 *                            of consecutive tile rows, to the ranks that fall short of the mean: the largest cost of any
 *                            rank (tiles + its own prepare, prep_permille/1000 tiles per 128 columns of its plane matrix;
 *                            < 0: the default) is smallest.  dst >= 0 names the rank that will RECEIVE the others' rows:
 *                            it sends nothing, so it takes dst_bonus_permille (< 0: the default -- 120 where a rank holds at least 16 tile rows, else 0) thousandths of a
 *                            rank's mean tile count more than the others, whose step only ends when their last part has
 *                            arrived; dst < 0: every rank keeps its rows.  Plain dsh_balance_rows ranges when n > 32 768
 *                            or a rank would hold fewer than two tile rows.  tab_out = NULL: only the size (words_out).
 *   dsh_rowsets_from_bounds  contiguous bounds[world + 1] as a table (3 + 2 world words): any alignment
 *   dsh_rowsets_rank         the segments {b0, e0, b1, e1, ...} of one rank, its pairs and its 128 x 128 tiles
 * The layout of every rank's buffer follows from (table, nparts, dst) alone:
 *   - the destination computes its own rows in place (d_local = d_final + the offset of its first row) as ONE part;
 *   - a rank with extra segments, or with a range of fewer than 1024 rows per part (span <= 1 GiB), goes ROW-SORTED: every
 *     segment key-ordered as one run (a range that reaches far down the triangle as two: its last rows on their own),
 *     d_local holds the rows in that order; the destination stages what it receives and puts the rows that are complete
 *     into place (one contiguous copy per row) behind every round, on a stream of its own;
 *   - longer ranges hold consecutive rows, received in place.
 * PARTS are units of completion (runs of whole tile rows, final in order; at most nparts -- a row-sorted rank whose parts
 * announce themselves from inside k_finalize cuts every tile row a part); what travels are MESSAGES: the exchange runs in
 * nparts ROUNDS, round q = one grouped ncclSend/ncclRecv of message q of every source, the q-th nparts-th of its buffer,
 * sent as soon as the part that holds its last value is final.  A round lasts as long as its largest message; with the
 * spans of dsh_balance_rowsets about equal no link waits for another's.
 * dsh_exchange_rows_device_async computes rank `rank`'s rows (enqueued; every part announces its completion: a flag written from
 * inside k_finalize, or an event between launches -- option finalize_signal), dsh_exchange_collect_async
 * enqueues the rounds on the copy stream; every rank calls both with the same arguments;
 * dsh_comm_wait completes them.  dsh_exchange_mode tells how a rank's buffer is laid out (rowsorted 0/1, parts at nparts) and how
 * many floats d_local must hold.  dsh_exchange_place_device does, for ONE source rank and without a communicator, what
 * the destination does with that rank's buffer (tests and single-GPU timing of an N-rank plan).
 * dsh_dist_collect(bounds = NULL) runs this pair over dsh_balance_rowsets' table. */
int dsh_balance_rowsets(uint64_t n, uint32_t world, int prep_permille, int dst, int dst_bonus_permille, uint64_t *tab_out,
                        uint32_t cap_words, uint32_t *words_out);
int dsh_rowsets_from_bounds(const uint64_t *bounds, uint32_t world, uint64_t *tab_out /* [3 + 2 world] */);
int dsh_rowsets_rank(uint64_t n, const uint64_t *rowsets, uint32_t rank, uint64_t *segs_out /* [2 cap_segs] or NULL */, uint32_t cap_segs,
                     uint32_t *nsegs_out, uint64_t *pairs_out, uint64_t *tiles_out);
int dsh_exchange_mode(uint64_t n, const uint64_t *rowsets, int rank, uint32_t nparts, int dst, int *rowsorted,
                      uint32_t *nparts_out, uint64_t *local_floats_out);
int dsh_exchange_rows_device_async(dsh_ctx *ctx, int estim, int result_type, int k, const uint64_t *rowsets, int rank,
                                   uint32_t nparts, int dst, void *d_local);
int dsh_exchange_collect_async(dsh_ctx *ctx, uint64_t n, const uint64_t *rowsets, uint32_t nparts, const void *d_local,
                               void *d_final, int dst);
int dsh_exchange_place_device(dsh_ctx *ctx, const uint64_t *rowsets, int src, uint32_t nparts, int dst,
                              const void *d_src_local, void *d_final);
/* Diagnostics of the exchange on ONE GPU (tests/test_gpu_multirank.py, tools/interference_probe.py):
 *   dsh_exchange_probe_parts_async  after dsh_exchange_rows_device_async with the same (table, rank, nparts, dst): enqueues
 *                        on the copy stream, for every part of the rank's call, the part's gate (the flag k_finalize
 *                        sets / the event) and behind it a copy KERNEL of the part's share of d_local into d_probe at the
 *                        same offsets -- plain loads through the L2s while k_finalize is still running, exactly what an
 *                        RCCL send kernel does with the part (the copy engine of a hipMemcpy reads memory instead).
 *                        dsh_wait / dsh_comm_wait completes it.  d_probe: as many floats as d_local.
 *                        On a context that holds a communicator of ONE rank (dsh_comm_init(.., 0, 1)) the reader is
 *                        librccl itself: the rank's buffer travels as dsh_exchange_collect_async would send it -- nparts
 *                        messages, each behind the gate of the part that holds its last value, one grouped call per
 *                        message -- by ncclSend to the rank itself paired with the ncclRecv into d_probe.
 *   dsh_diag_spin_start  occupies `nblocks` workgroups of `threads` lanes and `lds_bytes` of LDS each with a kernel that
 *                        polls a word of host memory -- what an RCCL receive kernel does while its peers have nothing to
 *                        send -- on a stream of its own, until dsh_diag_spin_stop or max_ms (<= 10 000) have passed:
 *                        measures what such a kernel costs the tile kernel beside it (option xch_recv_gate). */
int dsh_exchange_probe_parts_async(dsh_ctx *ctx, uint64_t n, const uint64_t *rowsets, int rank, uint32_t nparts, int dst,
                                   const void *d_local, void *d_probe);
int dsh_diag_spin_start(dsh_ctx *ctx, uint32_t nblocks, uint32_t threads, uint32_t lds_bytes, uint32_t max_ms);
int dsh_diag_spin_stop(dsh_ctx *ctx);
int dsh_comm_available(void);
int dsh_comm_library(char *path_out, size_t cap, int *version_out);
int dsh_comm_unique_id(void *id_out);
int dsh_comm_init(dsh_ctx *ctx, const void *unique_id, int rank, int world);
int dsh_comm_destroy(dsh_ctx *ctx);
int dsh_comm_rank(const dsh_ctx *ctx, int *rank, int *world);
int dsh_comm_wait(dsh_ctx *ctx);
int dsh_collect_spans(dsh_ctx *ctx, uint64_t n, const uint64_t *bounds, const void *d_local, void *d_final, int dst);
int dsh_collect_spans_async(dsh_ctx *ctx, uint64_t n, const uint64_t *bounds, const void *d_local, void *d_final, int dst);
int dsh_allgather_device(dsh_ctx *ctx, const void *d_send, uint64_t bytes_per_rank, void *d_recv);
int dsh_dist_collect(dsh_ctx *ctx, int estim, int result_type, int k, const uint64_t *bounds, int dst, float *out);

/* ---- helpers shared by every host (C++ CLI, Python, a patched dashing) -------------------- */
/* number of packed elements of rows [row_begin,row_end) of an n x n upper triangle */
uint64_t dsh_tri_span(uint64_t n, uint64_t row_begin, uint64_t row_end);
/* index(i,j) of distmat/distmat.h:260-264 */
uint64_t dsh_tri_index(uint64_t n, uint64_t i, uint64_t j);
/* Split rows [0,n) into nparts contiguous ranges of near-equal pair count, boundaries aligned
 * to `align` rows (the kernel tile, 128, keeps every rank on whole tile rows).
 * bounds_out[0..nparts] receives the boundaries (bounds_out[0]=0, bounds_out[nparts]=n). */
int dsh_partition_rows(uint64_t n, uint32_t nparts, uint32_t align, uint64_t *bounds_out);

/* Row ranges for the ranks of a multi-GPU run (or the devices of the CLI): bounds on 128-row boundaries that
 * minimise the largest number of 128 x 128 tiles any part computes (triangle of its rows + the rectangle
 * to their right).  Each range is then one dsh_dist_rows* call whose result is one contiguous span of the
 * final packed triangle -- the ranks' spans concatenate, nothing is re-ordered. */
int dsh_balance_rows(uint64_t n, uint32_t nparts, uint64_t *bounds_out);

/* Page-locked host memory for the host-buffer entry points (dsh_dist_rows, dsh_upload_sketches,
 * dsh_sketch_batch): with such buffers the copies are direct DMA at PCIe rate instead of going
 * through the runtime's staging of pageable memory.  Optional -- any host pointer works. */
void *dsh_alloc_host(size_t bytes);
void dsh_free_host(void *p);

/* ---- instrumentation ---------------------------------------------------------------------- */
/* Milliseconds spent in the dominant kernel (all-pairs AND+popcount) during the last
 * dsh_dist_* call on this ctx, measured with HIP events on the ctx stream; launches = number
 * of launches of that kernel in the call.  Enabled by dsh_set_profiling(ctx, 1) (adds event
 * records + one sync at the end of the call). */
int dsh_set_profiling(dsh_ctx *ctx, int enable);
int dsh_last_kernel_ms(dsh_ctx *ctx, double *pair_kernel_ms, double *finalize_kernel_ms,
                       double *prepare_ms, uint32_t *pair_kernel_launches);
/* (profiling on) the parts of the last call with parts (dsh_exchange_rows_device_async, dsh_dist_rows_parts_device_async):
 * when each became final, in ms from the start of the call (prepare included), and how many floats of the rank's buffer it
 * holds -- what a model of the pipelined exchange needs (tools/shard_model.py, bench.py --gpus N). */
int dsh_last_part_info(dsh_ctx *ctx, double *ready_ms /* [cap] or NULL */, uint64_t *floats /* [cap] or NULL */, uint32_t cap,
                       uint32_t *nparts_out);
/* Profiling aid: after a compare call with dsh_set_profiling(ctx, 1) and the option "finalize_timing" = 1 (the
 * s_memtime-stamped instance of k_finalize; results unchanged), out16 = shader-clock cycles summed over the waves that
 * finished, per phase [0..5] {prologue + loads issued, histogram columns, list joins, fix-ups, estimator, result + store};
 * [6] such waves; [7] their lanes; sums over lanes of [8] MLE iterations, [9] live bins, [10] iterations x bins; sums over
 * waves of the per-wave maxima [11] iterations, [12] bins, [13] their product (what a wave pays); [14..15] zero. */
int dsh_finalize_phase_cycles(dsh_ctx *ctx, uint64_t *out16);
/* Options; returns DSH_EINVAL for unknown names or values.  None changes a result (tests/test_gpu_compare.py asserts
 * byte-identical output over their ranges).  The tuning knobs of rounds 2-5 whose A/B was decided are gone together with
 * their losing arms (profiles/HISTORY.md has the measurements); what is left is what a caller or a first run on other
 * hardware needs:
 *   resources     "cum_budget_bytes"        scratch for the pair counts C(v) (default 8 GiB): larger jobs run in bands
 *                 "knn_square_budget_bytes" all-vs-all dsh_knn keeps an n x n float matrix in HBM up to this size (96 GiB)
 *                 "threshold_band_bytes"    dsh_dist_threshold* computes bands of whole rows of at most this much float32 (1 GiB)
 *                 "cluster_chunk"           dsh_cluster_pairs / dsh_cluster_csr unite at most this many edges per launch (2^20)
 *                 "greedy_band_rows"        a band of dsh_greedy_threshold* holds at most this many rows (4096; 1..8192)
 *                 "stats_route"             -1 auto | 0 dense | 1 pairs: how dsh_group_stats* computes the intra-group values
 *                 "linkage_budget_bytes"    the cell matrices of a batch of components of dsh_linkage_* (8 GiB)
 *                 "linkage_route"           -1 auto | 0 dense | 1 pairs: how dsh_linkage_threshold* fills them
 *                 "linkage_partition"       1 | 0: 0 = the whole collection as ONE component of dsh_linkage_*
 *                 "linkage_lds_max"         0..6144 (default 4096): components of dsh_linkage_* up to this size keep their
 *                                           per-row state in LDS, larger ones in global scratch
 *                 "derive_chunk_bytes"      the host forms of dsh_fold / dsh_upload_sketches_folded move at most this many bytes
 *                                           of source rows per step (256 MiB; at least one row)
 *                 "curve_scratch_bytes"     dsh_union_curve* runs batches of orders whose deltas, start rows and counters
 *                                           stay within this (256 MiB; at least one order)
 *                 "curve_segment"           members per segment of an order of dsh_union_curve*; 0 (default) = the planner's
 *   layout        "sort"                    -1 auto | 0 | 1: key-ordered plane columns (0 = identity: the slow, simple layout)
 *                 "range_sort_min_rows"     row ranges shorter than this keep the cached identity layout (default 1024)
 *                 "emax" / "elow"           caps of the listed upper / lower register tail, 0..255, -1 auto (per precision);
 *                                           0 / 0 = bit-planes over the whole value range (adversarial register laws)
 *   tile kernel   "kc"                      0 auto | 16 | 32 k-rows per LDS stage (auto: 16 with three work items per
 *                                           workgroup; with two, 32 where a plane has at least 32 words)
 *                 "pair_groups"             0 auto | 2 | 3 work items per workgroup of 256 x that many threads (waves per
 *                                           SIMD); auto = 3, or 2 where kc = 32 is asked for.  3 needs 16-row stages (LDS):
 *                                           with kc = 32 the next compare call fails with DSH_EINVAL.  A round of the
 *                                           kernel is 256 x pair_groups items.  Under auto a launch of at most 512 items
 *                                           (one round of two) still runs two per workgroup; 3 given by name always
 *                                           runs three.  Results do not depend on it.
 *                 "nsplit"                  pieces per tile, 0 auto (work items of at most 64 chunks)
 *                 "overflow_frag_permille"  0..1000 (default 500): a band whose one-plane work items number at most that
 *                                           share of a round above a multiple of a round has the items left over cut into
 *                                           fragments that ADD their counts; 0 = never
 *                 "sparse_planes"           -1 auto | 0 off | 1 | 2: a tile's top one or two bit-planes are counted from
 *                                           the positions of the few registers at or above the plane's threshold instead
 *                                           of by the tile kernel (kernels_sparseplane.hip), wherever no sketch of the
 *                                           tile's two blocks has more than "sparse_cap" of them; auto = at p >= 13 in
 *                                           launches of more than 512 planes.  Triangle calls on key-ordered columns only.
 *                                           Results do not depend on it.
 *                 "sparse_cap"              0..2040 (default 1280): the longest such set a routed plane may have
 *                 "sparse_sided"            -1 auto | 0 off | 1 forced: a plane of a tile is counted from position lists
 *                                           wherever ONE of its two blocks has every set -- registers at or above the
 *                                           threshold, or below it -- within "sparse_cap"; the other block only serves as
 *                                           a table.  Planes leave both ends of a tile's range, any number of them.  auto =
 *                                           where "sparse_planes" is -1 and its rule routes; forced: at p >= 13 whatever
 *                                           the size of the launch.  Off for a call whose "sparse_cap" is not the one the
 *                                           per-sketch pass of the attached matrix ran with.  Results do not depend on it.
 *                 "sparse_lds"              1 (default) | 0: up to p = 15 the counting kernel stages a word of the block's
 *                                           position table in LDS; 0 = it gathers from global memory, as at p = 16
 *                 "sparse_run"              0..65536 (default 0 = 4, the measured one): the items a workgroup of that LDS
 *                                           placement takes one behind the other, staging the table only where it changes;
 *                                           1 = one item per workgroup.  Results do not depend on it.
 *                 "sparse_words"            0 (default) | 1 | 2: the words of the table -- 32 columns each -- a workgroup
 *                                           of that placement stages side by side and a lane gathers in one LDS read;
 *                                           0 = 1, the faster one where it was measured (the pair leaves room for one
 *                                           workgroup a CU).  2 needs p <= 14, where the pair fits a CU's LDS: with it a
 *                                           compare call at p = 15 fails with DSH_EINVAL.  Results do not depend on it.
 *   exchange      "part_band_tiles"         a part of at least this many tiles also ends a launch of the tile kernel (2048)
 *                 "xch_tail_bands"          0..8 (default 2): a job with parts of at most 64 rounds has its tile kernel cut
 *                                           at whole rounds into a head and this many tails, so that the head's parts
 *                                           travel while the tails compute
 *                 "xch_recv_gate"           -1 auto | 0 | 1: the destination posts its receives behind its first tile
 *                                           kernel instead of at once (a waiting receive kernel beside the tile kernel
 *                                           costs it 2-14 %, profiles/rd6a/interference_probe.jsonl); auto = for a job
 *                                           of one launch of at most 8 rounds, whose peers have nothing to send earlier
 *                 "finalize_signal"         -1 auto | 0 | 1: parts announce themselves from inside ONE k_finalize launch
 *                                           per band (flags + hipStreamWaitValue32) instead of one launch and one event
 *                                           per part; auto = where the device supports stream wait-value
 *   profiling     "finalize_timing"         the s_memtime-stamped instance of k_finalize (same results)
 *                 "finalize_stop"           1..4: k_finalize leaves after a phase and stores a dummy -- CHANGES results;
 *                                           accepted only while dsh_set_profiling is on, cleared when it is switched off
 * ("pair_mfma" exists only in a library built with `make WHATIF=1`: the matrix-core what-if the north star excludes.) */
int dsh_set_option(dsh_ctx *ctx, const char *name, int64_t value);
/* Derived state of the last prepared sketch matrix: "planes" (dense bit-planes used), "vlo",
 * "vhi", "pbase", "threshold", "emax", "elow", "kc", "pair_groups" (as the last prepare put them into effect), "pair_round" (work items per round of the last dist call's first launch of the tile kernel: 256 x the items per workgroup it ran with), "tile", "npad", "kpad", "cum_bytes", "sorted", "ncols", "lockstep", "tiles", "bands", "items" (work items of the tile kernel), "sparse_items" ((tile, plane) items counted from position lists instead: option "sparse_planes"), "sparse_plane_us" (with profiling on: the device time of their counting kernel in the last dist call; it is part of the pair phase of dsh_last_kernel_ms), "sparse_sided_items" (those of them that the option "sparse_sided" planned), "sparse_transposed_items" (those whose lists are the column block's), "sparse_slabs" ((block, plane) slabs -- a table and position lists -- the last dist call's items read), "sparse_table_slabs" ((block, plane) tables of the last dist call built without lists), "sparse_table_fills" (table words the LDS placement of the counting kernel staged in the last dist call's launches: four per table; 0 where the table is gathered), "sparse_run" (the option in effect: 0 reads as the default), "sparse_words" (the option in effect for the attached matrix: 1 or 2; 0 where the table is gathered), "sparse_planes", "sparse_sided", "sparse_cap",
 * "words_per_plane", "avg_tile_planes_x100" (of the last dist call), "frag_items", "parts_done", "parts_signalled",
 * "place_kernel_us" (with profiling on: device time of the last dsh_exchange_place_device's placement kernel),
 * "sketch_kernel_us" / "fastx_decode_us" (with profiling on: k_sketch / the FASTA-FASTQ decode kernels of the last sketch call),
 * "stats_route" (the route the last dsh_group_stats* call took: 0 dense, 1 pairs; -1 before the first), "linkage_route" (the same
 * for the last dsh_linkage_threshold* call), "mst_rounds" (the rounds of the last dsh_mst* call that emitted an edge),
 * "mst_band_us" (with profiling on: the device time of its k_mst_band launches). */
int dsh_get_info(dsh_ctx *ctx, const char *name, int64_t *out);
/* HIP stream of the ctx as a void* (hipStream_t) so a host framework can order its own work.
 * Every *_device entry point runs on THIS stream and (except the *_async forms) returns after its work has
 * completed, so results are ready for any other stream on return.  The other direction is the caller's
 * job: whatever it enqueued on its own streams that touches a buffer passed in (filling d_out, producing
 * d_regs or d_seq, an RCCL gather into a staging buffer) must have completed on the host -- or be ordered
 * before this stream's work with dsh_wait_event -- before the call. */
void *dsh_stream(dsh_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* DASHING_HIP_H_ */
