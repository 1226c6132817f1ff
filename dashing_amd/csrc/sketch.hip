// sketch.hip -- the sketch waist of libdashing_hip.so: dsh_sketch_batch{,_async,_device}, dsh_sketch_records{,_async,_device}
// and dsh_sketch_fastx_batch_async.  Every entry point is the same sequence -- check, source (a host span staged, or a device
// pointer checked), plan (sketch_plan.h: pure host arithmetic), launch, invalidate, and the wait or download its contract
// has -- and each step is written once here.  The kernels are kernels_sketch.hip and kernels_fastx.hip.
#include <algorithm>
#include <cstring>

#include "ctx.h"

using namespace dsh;

namespace {

// What every sketch entry point refuses, all of it before anything is enqueued: off[n + 1] are the genomes' or records'
// offsets, their rows the slots [first_slot, first_slot + n), which the work lists keep in 32 bits.  Binds the device.
int sketch_enter(dsh_ctx *c, const uint64_t *off, uint32_t n, uint64_t first_slot, int k)
{
    if (!c || (!off && n)) return DSH_EINVAL;
    if (k < 1 || k > 32) return fail(c, DSH_EINVAL, "k=%d outside [1,32]", k);
    if (!c->have_sketches || c->regs != (const uint8_t *)c->regs_own.ptr)
        return fail(c, DSH_ESTATE, "dsh_sketches_alloc first");
    if (!slots_ok(first_slot, n, c->n)) return fail(c, DSH_EINVAL, "slots out of range");
    for (uint32_t g = 0; g < n; ++g)
        if (off[g + 1] < off[g]) return fail(c, DSH_EINVAL, "offsets not monotone at %u", g);
    if (first_slot + n > 0xFFFFFFFFull) return fail(c, DSH_EINVAL, "slots beyond 2^32");
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

// per-record sketches: one row per record, overwritten (plan_records)
int sketch_records(dsh_ctx *c, const uint8_t *d_seq, const uint64_t *off, uint32_t n, uint64_t first_slot, int k, int canon)
{
    uint8_t *regs = (uint8_t *)c->regs_own.ptr;
    const int p = c->p;
    std::vector<RecRun> runs;
    std::vector<RecSeg> segs;
    std::vector<uint32_t> zero;  // rows of the long records
    std::vector<SketchWork> work;
    if (!plan_records(off, n, first_slot, k, p, runs, segs, zero, work)) {
        HIPCHK(c, hipMemsetAsync(regs + (first_slot << p), 0, (size_t)n << p, c->stream));
        return run_sketch_work(c, d_seq, work, k, canon);
    }
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
    return run_sketch_work(c, d_seq, work, k, canon);
}

typedef int (*SketchFn)(dsh_ctx *, const uint8_t *, const uint64_t *, uint32_t, uint64_t, int, int);

// the _async forms: the span of a host sequence staged, everything enqueued, nothing waited for
int from_host(dsh_ctx *c, SketchFn sketch, const uint8_t *seq, const uint64_t *off, uint32_t n, uint64_t first_slot, int k, int canon)
{
    int rc = sketch_enter(c, off, n, first_slot, k);
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
    int rc = sketch_enter(c, off, n, first_slot, k);
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

// raw FASTA / FASTQ bytes decoded on the device into seqbuf (kernels_fastx.hip), then sketched as genomes
int dsh_sketch_fastx_batch_async(dsh_ctx *c, const uint8_t *raw, const uint64_t *genome_off, const uint64_t *raw_len,
                                 uint32_t n_genomes, uint64_t first_slot, int k, int canon, uint32_t *status_out)
{
    int rc = sketch_enter(c, genome_off, n_genomes, first_slot, k);
    if (rc || n_genomes == 0) return rc;
    const uint64_t lo = genome_off[0];
    const size_t bytes = (size_t)(genome_off[n_genomes] - lo);
    if (!raw_len || (bytes && !raw)) return DSH_EINVAL;
    std::vector<FastxGenome> gen;
    std::vector<FastxChunk> chunks;
    uint32_t bad = 0;
    switch (plan_fastx(raw, genome_off, raw_len, n_genomes, gen, chunks, &bad)) {
    case kFastxPlanRegion:
        return fail(c, DSH_EINVAL, "genome %u: its region must start on a multiple of 32 and hold its %llu raw bytes", bad, (unsigned long long)raw_len[bad]);
    case kFastxPlanTooLarge:
        return fail(c, DSH_EINVAL, "batch too large");
    }
    HIPCHK(c, c->sketch.rawbuf.ensure(bytes + 256));
    HIPCHK(c, c->sketch.seqbuf.ensure(bytes + 256));
    if (bytes) HIPCHK(c, hipMemcpyAsync(c->sketch.rawbuf.ptr, raw + lo, bytes, hipMemcpyHostToDevice, c->stream));
    const size_t gbytes = gen.size() * sizeof(FastxGenome), cbytes = chunks.size() * sizeof(FastxChunk);
    // (the previous batch's tables have long been uploaded unless calls come back to back)
    HIPCHK(c, c->sketch.fx.room(gbytes + cbytes));
    std::memcpy(c->sketch.fx.ptr(), gen.data(), gbytes);
    if (cbytes) std::memcpy((uint8_t *)c->sketch.fx.ptr() + gbytes, chunks.data(), cbytes);
    HIPCHK(c, c->sketch.fx_tab.ensure(gbytes + cbytes));
    HIPCHK(c, launch_upload(c->stream, c->sketch.fx_tab.ptr, c->sketch.fx.ptr(), gbytes + cbytes));
    HIPCHK(c, c->sketch.fx.sent(c->stream));
    HIPCHK(c, c->sketch.fx_summ.ensure(std::max<size_t>(chunks.size(), 1) * sizeof(FastxSumm)));
    HIPCHK(c, c->sketch.fx_state.ensure(std::max<size_t>(chunks.size(), 1) * sizeof(uint4)));
    HIPCHK(c, c->sketch.fx_declen.ensure(gen.size() * sizeof(uint64_t)));
    // [status words | length fingerprints]: one buffer, cleared by one memset
    const size_t st_bytes = (gen.size() * sizeof(uint32_t) + 7) & ~(size_t)7;
    HIPCHK(c, c->sketch.fx_status.ensure(st_bytes + gen.size() * sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->sketch.fx_status.ptr, 0, st_bytes + gen.size() * sizeof(unsigned long long), c->stream));
    if (c->profiling) c->ev_used = 0;
    DeviceTimer ft(c, c->stream);  // (profiling: the decode kernels alone, dsh_get_info "fastx_decode_us")
    HIPCHK(c, launch_fastx_decode(c->stream, (const uint8_t *)c->sketch.rawbuf.ptr, (const FastxChunk *)((const uint8_t *)c->sketch.fx_tab.ptr + gbytes),
                                  (uint32_t)chunks.size(), (const FastxGenome *)c->sketch.fx_tab.ptr, n_genomes, (FastxSumm *)c->sketch.fx_summ.ptr,
                                  (uint4 *)c->sketch.fx_state.ptr, (uint64_t *)c->sketch.fx_declen.ptr, (uint32_t *)c->sketch.fx_status.ptr,
                                  (unsigned long long *)((uint8_t *)c->sketch.fx_status.ptr + st_bytes), (uint8_t *)c->sketch.seqbuf.ptr));
    ft.stop(c->fastx_ms);
    if (status_out)
        HIPCHK(c, hipMemcpyAsync(status_out, c->sketch.fx_status.ptr, gen.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    const std::vector<uint64_t> off = rebased(genome_off, n_genomes, lo);
    if ((rc = sketch_genomes(c, (const uint8_t *)c->sketch.seqbuf.ptr, off.data(), n_genomes, first_slot, k, canon))) return rc;
    invalidate(c);
    return DSH_OK;
}

}  // extern "C"
