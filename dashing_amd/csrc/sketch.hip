// sketch.hip -- the sketch waist of libdashing_hip.so: dsh_sketch_batch{,_async,_device}, dsh_sketch_records{,_async,_device},
// dsh_sketch_fastx_batch_async and dsh_sketch_fastx_records.  Every entry point is the same sequence -- check, source (a host span staged, or a device
// pointer checked), plan (sketch_plan.h: pure host arithmetic), launch, invalidate, and the wait or download its contract
// has -- and each step is written once here.  The kernels are kernels_sketch.hip and kernels_fastx.hip.
#include <algorithm>
#include <cstring>

#include "ctx.h"

using namespace dsh;

namespace {

// What every sketch entry point refuses, all of it before anything is enqueued: off[n + 1] are the genomes' or records'
// offsets, their rows the slots [first_slot, first_slot + n_slots), which the work lists keep in 32 bits.  Binds the device.
int sketch_enter(dsh_ctx *c, const uint64_t *off, uint32_t n, uint64_t first_slot, uint64_t n_slots, int k)
{
    if (!c || (!off && n)) return DSH_EINVAL;
    if (k < 1 || k > 32) return fail(c, DSH_EINVAL, "k=%d outside [1,32]", k);
    if (!c->have_sketches || c->regs != (const uint8_t *)c->regs_own.ptr)
        return fail(c, DSH_ESTATE, "dsh_sketches_alloc first");
    if (!slots_ok(first_slot, n_slots, c->n)) return fail(c, DSH_EINVAL, "slots out of range");
    for (uint32_t g = 0; g < n; ++g)
        if (off[g + 1] < off[g]) return fail(c, DSH_EINVAL, "offsets not monotone at %u", g);
    if (first_slot + n_slots > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "slots beyond 2^32");
    return bind(c);
}

// off[0 .. n] counted from `base`
std::vector<uint64_t> rebased(const uint64_t *off, uint32_t n, uint64_t base)
{
    std::vector<uint64_t> local(n + 1);
    for (uint32_t g = 0; g <= n; ++g) local[g] = off[g] - base;
    return local;
}

// Ships only [off[0], off[n]) of a host sequence, to seqbuf: 32-aligned on the device side (the span keeps its place
// within 32 bytes) and padded so that every lane's 64-byte read is in bounds.  `local`: the offsets inside seqbuf.
int stage_host_span(dsh_ctx *c, const uint8_t *seq, const uint64_t *off, uint32_t n, std::vector<uint64_t> &local)
{
    const uint64_t lo = off[0], hi = off[n], shift = lo & 31;
    if (hi > lo && !seq) return fail(c, DSH_EINVAL, "seq is NULL");
    HIPCHK(c, c->sketch.seqbuf.ensure((size_t)(hi - lo) + shift + 256));
    if (hi > lo)
        HIPCHK(c, hipMemcpyAsync((uint8_t *)c->sketch.seqbuf.ptr + shift, seq + lo, (size_t)(hi - lo), hipMemcpyHostToDevice, c->stream));
    local = rebased(off, n, lo - shift);
    return DSH_OK;
}

int device_seq_check(dsh_ctx *c, const void *d_seq)
{
    if (!d_seq || ((uintptr_t)d_seq & 31)) return fail(c, DSH_EINVAL, "d_seq must be 32-byte aligned and padded by 128 bytes");
    return DSH_OK;
}

// upload a k_sketch work list and launch it
int run_sketch_work(dsh_ctx *c, const uint8_t *d_seq, const std::vector<SketchWork> &work, int k, int canon)
{
    if (work.empty()) return DSH_OK;
    // the work list travels through page-locked staging (rewritten only after its previous upload has run),
    // so nothing here waits: the blocking entry points synchronise, the _async ones return
    HIPCHK(c, c->sketch.work.room(work.size() * sizeof(SketchWork)));
    std::memcpy(c->sketch.work.ptr(), work.data(), work.size() * sizeof(SketchWork));
    HIPCHK(c, c->sketch.workbuf.ensure(work.size() * sizeof(SketchWork)));
    HIPCHK(c, launch_upload(c->stream, c->sketch.workbuf.ptr, c->sketch.work.ptr(), work.size() * sizeof(SketchWork)));
    HIPCHK(c, c->sketch.work.sent(c->stream));
    if (c->profiling) c->ev_used = 0;
    DeviceTimer t(c, c->stream);  // k_sketch alone, on the stream it runs on
    HIPCHK(c, launch_sketch(c->stream, d_seq, (const SketchWork *)c->sketch.workbuf.ptr,
                            (uint32_t)work.size(), k, c->p, canon, (uint8_t *)c->regs_own.ptr));
    t.stop(c->sketch_ms);
    return DSH_OK;
}

// genomes max-merged into their rows; off is relative to d_seq (32-byte aligned, padded by 128 bytes)
int sketch_genomes(dsh_ctx *c, const uint8_t *d_seq, const uint64_t *off, uint32_t n, uint64_t first_slot, int k, int canon)
{
    std::vector<SketchWork> work;
    plan_genomes(off, n, first_slot, k, c->p, work);
    return run_sketch_work(c, d_seq, work, k, canon);
}

// plan_records' lists (appended to by every call of it)
struct RecordLists {
    std::vector<RecRun> runs;
    std::vector<RecSeg> segs;
    std::vector<uint32_t> zero;  // rows of the long records
    std::vector<SketchWork> work;
};

// upload plan_records' lists and launch their kernels
int run_record_lists(dsh_ctx *c, const uint8_t *d_seq, const RecordLists &L, int k, int canon)
{
    uint8_t *regs = (uint8_t *)c->regs_own.ptr;
    const int p = c->p;
    const std::vector<RecRun> &runs = L.runs;
    const std::vector<RecSeg> &segs = L.segs;
    const std::vector<uint32_t> &zero = L.zero;
    // one upload: runs, segments, rows to clear
    const size_t rb = runs.size() * sizeof(RecRun), sb = segs.size() * sizeof(RecSeg), zb = zero.size() * sizeof(uint32_t);
    const size_t so = (rb + 15) & ~(size_t)15, zo = so + ((sb + 15) & ~(size_t)15), tot = zo + zb;
    if (tot) {
        HIPCHK(c, c->sketch.rec.room(tot));
        HIPCHK(c, c->sketch.recbuf.ensure(tot));
        uint8_t *h = (uint8_t *)c->sketch.rec.ptr();
        if (rb) std::memcpy(h, runs.data(), rb);
        if (sb) std::memcpy(h + so, segs.data(), sb);
        if (zb) std::memcpy(h + zo, zero.data(), zb);
        HIPCHK(c, launch_upload(c->stream, c->sketch.recbuf.ptr, c->sketch.rec.ptr(), tot));
        HIPCHK(c, c->sketch.rec.sent(c->stream));
    }
    const uint8_t *d = (const uint8_t *)c->sketch.recbuf.ptr;
    HIPCHK(c, launch_zero_rows(c->stream, (const uint32_t *)(d + zo), (uint32_t)zero.size(), p, regs));
    HIPCHK(c, launch_sketch_records(c->stream, d_seq, (const RecRun *)d, (uint32_t)runs.size(), (const uint2 *)(d + so), k, p,
                                    canon, regs));
    return run_sketch_work(c, d_seq, L.work, k, canon);
}

// per-record sketches: one row per record, overwritten (plan_records)
int sketch_records(dsh_ctx *c, const uint8_t *d_seq, const uint64_t *off, uint32_t n, uint64_t first_slot, int k, int canon)
{
    RecordLists L;
    if (!plan_records(off, n, first_slot, k, c->p, L.runs, L.segs, L.zero, L.work)) {
        HIPCHK(c, hipMemsetAsync((uint8_t *)c->regs_own.ptr + (first_slot << c->p), 0, (size_t)n << c->p, c->stream));
        return run_sketch_work(c, d_seq, L.work, k, canon);
    }
    return run_record_lists(c, d_seq, L, k, canon);
}

typedef int (*SketchFn)(dsh_ctx *, const uint8_t *, const uint64_t *, uint32_t, uint64_t, int, int);

// the _async forms: the span of a host sequence staged, everything enqueued, nothing waited for
int from_host(dsh_ctx *c, SketchFn sketch, const uint8_t *seq, const uint64_t *off, uint32_t n, uint64_t first_slot, int k, int canon)
{
    int rc = sketch_enter(c, off, n, first_slot, n, k);
    if (rc || n == 0) return rc;
    std::vector<uint64_t> local;
    if ((rc = stage_host_span(c, seq, off, n, local))) return rc;
    if ((rc = sketch(c, (const uint8_t *)c->sketch.seqbuf.ptr, local.data(), n, first_slot, k, canon))) return rc;
    invalidate(c);
    return DSH_OK;
}

// the blocking forms: behind their _async form (rc), the wait and the rows where they are wanted
int finish_blocking(dsh_ctx *c, int rc, uint64_t first_slot, uint32_t n, uint8_t *regs_out)
{
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (a pageable `seq` was copied synchronously anyway)
    if (regs_out) return dsh_download_sketches(c, first_slot, n, regs_out);
    return DSH_OK;
}

// the _device forms: off is relative to d_seq; returns when the rows are written
int from_device(dsh_ctx *c, SketchFn sketch, const void *d_seq, const uint64_t *off, uint32_t n, uint64_t first_slot, int k, int canon)
{
    int rc = sketch_enter(c, off, n, first_slot, n, k);
    if (rc || n == 0) return rc;
    if ((rc = device_seq_check(c, d_seq))) return rc;
    if ((rc = sketch(c, (const uint8_t *)d_seq, off, n, first_slot, k, canon))) return rc;
    invalidate(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_sketch_batch_async(dsh_ctx *c, const uint8_t *seq, const uint64_t *genome_off, uint32_t n_genomes,
                           uint64_t first_slot, int k, int canon)
{
    return from_host(c, sketch_genomes, seq, genome_off, n_genomes, first_slot, k, canon);
}

int dsh_sketch_batch(dsh_ctx *c, const uint8_t *seq, const uint64_t *genome_off, uint32_t n_genomes,
                     uint64_t first_slot, int k, int canon, uint8_t *regs_out)
{
    return finish_blocking(c, dsh_sketch_batch_async(c, seq, genome_off, n_genomes, first_slot, k, canon), first_slot, n_genomes, regs_out);
}

int dsh_sketch_batch_device(dsh_ctx *c, const void *d_seq, const uint64_t *genome_off,
                            uint32_t n_genomes, uint64_t first_slot, int k, int canon)
{
    return from_device(c, sketch_genomes, d_seq, genome_off, n_genomes, first_slot, k, canon);
}

int dsh_sketch_records_async(dsh_ctx *c, const uint8_t *seq, const uint64_t *rec_off, uint32_t n_records, uint64_t first_slot,
                             int k, int canon)
{
    return from_host(c, sketch_records, seq, rec_off, n_records, first_slot, k, canon);
}

int dsh_sketch_records(dsh_ctx *c, const uint8_t *seq, const uint64_t *rec_off, uint32_t n_records, uint64_t first_slot, int k,
                       int canon, uint8_t *regs_out)
{
    return finish_blocking(c, dsh_sketch_records_async(c, seq, rec_off, n_records, first_slot, k, canon), first_slot, n_records, regs_out);
}

int dsh_sketch_records_device(dsh_ctx *c, const void *d_seq, const uint64_t *rec_off, uint32_t n_records, uint64_t first_slot,
                              int k, int canon)
{
    return from_device(c, sketch_records, d_seq, rec_off, n_records, first_slot, k, canon);
}

}  // extern "C"

namespace {

// What the two fastx entry points share.  fastx_plan: the decoder's tables, with its refusals (nothing is enqueued yet).
// fastx_stage: the raw bytes shipped to rawbuf, the tables -- and `extra` behind them -- uploaded to fx_tab, the scratch sized,
// the status words and length fingerprints cleared.  fastx_decode: the kernels, with the record index or without.
struct FastxCall {
    std::vector<FastxGenome> gen;
    std::vector<FastxChunk> chunks;
    size_t tab_bytes = 0;  // the tables in fx_tab: [genomes | chunks], then `extra`
    size_t st_bytes = 0;   // fx_status: [status words | length fingerprints]
};

int fastx_plan(dsh_ctx *c, const uint8_t *raw, const uint64_t *off, const uint64_t *raw_len, uint32_t n, FastxCall &fc)
{
    if (!raw_len || (off[n] > off[0] && !raw)) return DSH_EINVAL;
    uint32_t bad = 0;
    switch (plan_fastx(raw, off, raw_len, n, fc.gen, fc.chunks, &bad)) {
    case kFastxPlanRegion:
        return fail(c, DSH_EINVAL, "genome %u: its region must start on a multiple of 32 and hold its %llu raw bytes", bad, (unsigned long long)raw_len[bad]);
    case kFastxPlanTooLarge:
        return fail(c, DSH_EINVAL, "batch too large");
    }
    fc.tab_bytes = fc.gen.size() * sizeof(FastxGenome) + fc.chunks.size() * sizeof(FastxChunk);
    fc.st_bytes = (fc.gen.size() * sizeof(uint32_t) + 7) & ~(size_t)7;
    return DSH_OK;
}

int fastx_stage(dsh_ctx *c, const uint8_t *raw, const uint64_t *off, uint32_t n, const FastxCall &fc, const void *extra = nullptr,
                size_t extra_bytes = 0)
{
    const size_t bytes = (size_t)(off[n] - off[0]);
    HIPCHK(c, c->sketch.rawbuf.ensure(bytes + 256));
    HIPCHK(c, c->sketch.seqbuf.ensure(bytes + 256));
    if (bytes) HIPCHK(c, hipMemcpyAsync(c->sketch.rawbuf.ptr, raw + off[0], bytes, hipMemcpyHostToDevice, c->stream));
    const size_t gbytes = fc.gen.size() * sizeof(FastxGenome), cbytes = fc.chunks.size() * sizeof(FastxChunk);
    // (the previous batch's tables have long been uploaded unless calls come back to back)
    HIPCHK(c, c->sketch.fx.room(fc.tab_bytes + extra_bytes));
    std::memcpy(c->sketch.fx.ptr(), fc.gen.data(), gbytes);
    if (cbytes) std::memcpy((uint8_t *)c->sketch.fx.ptr() + gbytes, fc.chunks.data(), cbytes);
    if (extra_bytes) std::memcpy((uint8_t *)c->sketch.fx.ptr() + fc.tab_bytes, extra, extra_bytes);
    HIPCHK(c, c->sketch.fx_tab.ensure(fc.tab_bytes + extra_bytes));
    HIPCHK(c, launch_upload(c->stream, c->sketch.fx_tab.ptr, c->sketch.fx.ptr(), fc.tab_bytes + extra_bytes));
    HIPCHK(c, c->sketch.fx.sent(c->stream));
    HIPCHK(c, c->sketch.fx_summ.ensure(std::max<size_t>(fc.chunks.size(), 1) * sizeof(FastxSumm)));
    HIPCHK(c, c->sketch.fx_state.ensure(std::max<size_t>(fc.chunks.size(), 1) * sizeof(uint4)));
    HIPCHK(c, c->sketch.fx_declen.ensure(fc.gen.size() * sizeof(uint64_t)));
    // [status words | length fingerprints]: one buffer, cleared by one memset
    HIPCHK(c, c->sketch.fx_status.ensure(fc.st_bytes + fc.gen.size() * sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->sketch.fx_status.ptr, 0, fc.st_bytes + fc.gen.size() * sizeof(unsigned long long), c->stream));
    return DSH_OK;
}

int fastx_decode(dsh_ctx *c, const FastxCall &fc, const FastxRecIndex *ix)
{
    const size_t gbytes = fc.gen.size() * sizeof(FastxGenome);
    const uint8_t *raw = (const uint8_t *)c->sketch.rawbuf.ptr;
    const FastxGenome *gen = (const FastxGenome *)c->sketch.fx_tab.ptr;
    const FastxChunk *chunks = (const FastxChunk *)((const uint8_t *)c->sketch.fx_tab.ptr + gbytes);
    const uint32_t nchunks = (uint32_t)fc.chunks.size(), n = (uint32_t)fc.gen.size();
    FastxSumm *summ = (FastxSumm *)c->sketch.fx_summ.ptr;
    uint4 *state = (uint4 *)c->sketch.fx_state.ptr;
    uint64_t *declen = (uint64_t *)c->sketch.fx_declen.ptr;
    uint32_t *status = (uint32_t *)c->sketch.fx_status.ptr;
    unsigned long long *fingerprint = (unsigned long long *)((uint8_t *)c->sketch.fx_status.ptr + fc.st_bytes);
    uint8_t *out = (uint8_t *)c->sketch.seqbuf.ptr;
    if (c->profiling) c->ev_used = 0;
    DeviceTimer ft(c, c->stream);  // (profiling: the decode kernels alone, dsh_get_info "fastx_decode_us")
    if (ix) HIPCHK(c, launch_fastx_decode_records(c->stream, raw, chunks, nchunks, gen, n, summ, state, declen, status, fingerprint, out, *ix));
    else HIPCHK(c, launch_fastx_decode(c->stream, raw, chunks, nchunks, gen, n, summ, state, declen, status, fingerprint, out));
    ft.stop(c->fastx_ms);
    return DSH_OK;
}

}  // namespace

extern "C" {

// raw FASTA / FASTQ bytes decoded on the device into seqbuf (kernels_fastx.hip), then sketched as genomes
int dsh_sketch_fastx_batch_async(dsh_ctx *c, const uint8_t *raw, const uint64_t *genome_off, const uint64_t *raw_len,
                                 uint32_t n_genomes, uint64_t first_slot, int k, int canon, uint32_t *status_out)
{
    int rc = sketch_enter(c, genome_off, n_genomes, first_slot, n_genomes, k);
    if (rc || n_genomes == 0) return rc;
    FastxCall fc;
    if ((rc = fastx_plan(c, raw, genome_off, raw_len, n_genomes, fc))) return rc;
    if ((rc = fastx_stage(c, raw, genome_off, n_genomes, fc))) return rc;
    if ((rc = fastx_decode(c, fc, nullptr))) return rc;
    if (status_out)
        HIPCHK(c, hipMemcpyAsync(status_out, c->sketch.fx_status.ptr, fc.gen.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    const std::vector<uint64_t> off = rebased(genome_off, n_genomes, genome_off[0]);
    if ((rc = sketch_genomes(c, (const uint8_t *)c->sketch.seqbuf.ptr, off.data(), n_genomes, first_slot, k, canon))) return rc;
    invalidate(c);
    return DSH_OK;
}

// raw FASTA / FASTQ bytes decoded on the device WITH the record index, then every record of every accepted file sketched into
// its own row.  slot_ptr == NULL: the counts alone (passes A and B), nothing emitted or sketched.
int dsh_sketch_fastx_records(dsh_ctx *c, const uint8_t *raw, const uint64_t *file_off, const uint64_t *raw_len, uint32_t n_files,
                             const uint64_t *slot_ptr, int k, int canon, uint32_t *status_out, uint64_t *n_rec_out,
                             uint64_t *hdr_off_out)
{
    const bool count_only = !slot_ptr;
    if (!c || (n_files && (!file_off || !raw_len || !status_out || !n_rec_out))) return DSH_EINVAL;
    uint64_t total = 0;
    int rc;
    if (count_only) {
        if (k < 1 || k > 32) return fail(c, DSH_EINVAL, "k=%d outside [1,32]", k);
        rc = bind(c);
    } else {
        for (uint32_t f = 0; f < n_files; ++f)
            if (slot_ptr[f + 1] < slot_ptr[f]) return fail(c, DSH_EINVAL, "slot_ptr not monotone at %u", f);
        total = slot_ptr[n_files] - slot_ptr[0];
        rc = sketch_enter(c, file_off, n_files, slot_ptr[0], total, k);
    }
    if (rc || n_files == 0) return rc;
    FastxCall fc;
    if ((rc = fastx_plan(c, raw, file_off, raw_len, n_files, fc))) return rc;

    // the index.  rec0 travels behind the decoder's tables; fx_rec holds [dpos | rpos | nrec | cnt]
    std::vector<uint64_t> rec0(n_files + 1, 0);
    if (!count_only)
        for (uint32_t f = 0; f <= n_files; ++f) rec0[f] = slot_ptr[f] - slot_ptr[0];
    if ((rc = fastx_stage(c, raw, file_off, n_files, fc, rec0.data(), rec0.size() * sizeof(uint64_t)))) return rc;
    const size_t ib = std::max<size_t>((size_t)total, 1) * sizeof(uint64_t), nb = (size_t)n_files * 2 * sizeof(uint32_t);
    const size_t cb = std::max<size_t>(fc.chunks.size(), 1) * 3 * sizeof(uint32_t);
    HIPCHK(c, c->sketch.fx_rec.ensure(2 * ib + nb + cb));
    uint8_t *d = (uint8_t *)c->sketch.fx_rec.ptr;
    FastxRecIndex ix;
    ix.dpos = (uint64_t *)d;
    ix.rpos = (uint64_t *)(d + ib);
    ix.nrec = (uint32_t *)(d + 2 * ib);
    ix.cnt = (uint32_t *)(d + 2 * ib + nb);
    ix.rec0 = count_only ? nullptr : (const uint64_t *)((const uint8_t *)c->sketch.fx_tab.ptr + fc.tab_bytes);
    if ((rc = fastx_decode(c, fc, &ix))) return rc;

    // back: the verdicts (behind k_fastx_pad: the late ones are in), the counts, the decoded lengths, the index
    std::vector<uint32_t> status(n_files), nrec(2 * (size_t)n_files);
    std::vector<uint64_t> declen(n_files), pos(2 * (size_t)total);
    HIPCHK(c, hipMemcpyAsync(status.data(), c->sketch.fx_status.ptr, n_files * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(nrec.data(), ix.nrec, nb, hipMemcpyDeviceToHost, c->stream));
    if (total) {
        HIPCHK(c, hipMemcpyAsync(declen.data(), c->sketch.fx_declen.ptr, n_files * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(pos.data(), ix.dpos, (size_t)total * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(pos.data() + total, ix.rpos, (size_t)total * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (uint32_t f = 0; f < n_files; ++f) {
        status_out[f] = status[f];
        n_rec_out[f] = status[f] ? 0 : (uint64_t)((int64_t)nrec[2 * f] + fastx_tail_records(raw + file_off[f], raw_len[f], fc.gen[f].fmt, nrec[2 * f + 1]));
    }
    if (count_only) return DSH_OK;
    for (uint32_t f = 0; f < n_files; ++f)
        if (!status[f] && n_rec_out[f] != rec0[f + 1] - rec0[f])
            return fail(c, DSH_ERANGE, "file %u holds %llu records, its span %llu slots: no row was written, call again with the counts",
                        f, (unsigned long long)n_rec_out[f], (unsigned long long)(rec0[f + 1] - rec0[f]));

    // the accepted files' records, file after file, into one set of lists
    RecordLists L;
    std::vector<uint64_t> off;
    bool as_genomes = false;  // (p above kMaxPRecords: every record is k_sketch's, its row cleared here)
    for (uint32_t f = 0; f < n_files; ++f) {
        const uint64_t n = n_rec_out[f];
        if (status[f] || n == 0) continue;
        const uint64_t markers = std::min<uint64_t>(nrec[2 * f], n);
        const uint64_t *dpos = pos.data() + rec0[f], *rpos = pos.data() + total + rec0[f];
        fastx_record_offsets(dpos, markers, n, fc.gen[f].off + declen[f], off);
        if (!plan_records(off.data(), (uint32_t)n, slot_ptr[f], k, c->p, L.runs, L.segs, L.zero, L.work)) {
            as_genomes = true;
            HIPCHK(c, hipMemsetAsync((uint8_t *)c->regs_own.ptr + (slot_ptr[f] << c->p), 0, (size_t)n << c->p, c->stream));
        }
        if (!hdr_off_out) continue;
        const uint8_t *file = raw + file_off[f];
        for (uint64_t r = 0; r < n; ++r) {
            uint64_t at = r < markers ? rpos[r] - fc.gen[f].off : raw_len[f] - 1;  // (a FASTA marker IS the header character)
            if (fc.gen[f].fmt != 0) at = fastx_line_start(file, at);
            hdr_off_out[rec0[f] + r] = file_off[f] + at;
        }
    }
    const uint8_t *d_seq = (const uint8_t *)c->sketch.seqbuf.ptr;
    if ((rc = as_genomes ? run_sketch_work(c, d_seq, L.work, k, canon) : run_record_lists(c, d_seq, L, k, canon))) return rc;
    invalidate(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
}

}  // extern "C"
