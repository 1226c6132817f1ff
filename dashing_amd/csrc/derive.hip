// derive.hip -- dsh_fold*, dsh_upload_sketches_folded*, dsh_union_groups*: new sketches out of resident ones (DESIGN.md
// 4.9, kernels_derive.hip).  dsh_fold* and dsh_union_groups* read the resident rows and write the caller's buffer: nothing
// of the context's derived state is read or written.  dsh_upload_sketches_folded* writes resident rows and invalidates as
// dsh_upload_sketches does.  The host forms move rows through scratch of at most "derive_chunk_bytes" of source rows.
#include <algorithm>

#include "ctx.h"

using namespace dsh;

namespace {

int err_begin(dsh_ctx *c)
{
    HIPCHK(c, c->derive.err.ensure(sizeof(unsigned long long)));
    HIPCHK(c, hipMemsetAsync(c->derive.err.ptr, 0xFF, sizeof(unsigned long long), c->stream));
    return DSH_OK;
}

// the one wait of a call: the error word, then the stream is idle
int err_end(dsh_ctx *c, int src_p)
{
    unsigned long long e = ~0ull;
    HIPCHK(c, hipMemcpyAsync(&e, c->derive.err.ptr, sizeof e, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (e != ~0ull)
        return fail(c, DSH_EINVAL, "sketch %llu holds a register value above %d (= 64 - p + 1): not an HLL of precision %d (corrupt or foreign .hll?)",
                    e, 64 - src_p + 1, src_p);
    return DSH_OK;
}

uint64_t chunk_rows(const dsh_ctx *c, int src_p) { return std::max<uint64_t>(c->derive.chunk_bytes >> src_p, 1); }

int check_fold(dsh_ctx *c, uint64_t first, uint64_t n, int new_p)
{
    int rc = enter(c);
    if (rc) return rc;
    if (new_p < 4 || new_p > c->p) return fail(c, DSH_EINVAL, "new_p=%d outside [4,%d]", new_p, c->p);
    if (!slots_ok(first, n, c->n)) return fail(c, DSH_EINVAL, "slots [%llu,+%llu) out of range", (unsigned long long)first, (unsigned long long)n);
    return DSH_OK;
}

int check_upload(dsh_ctx *c, int src_p, uint64_t first, uint64_t n)
{
    if (!c) return DSH_EINVAL;
    if (!c->have_sketches || c->regs != (const uint8_t *)c->regs_own.ptr) return fail(c, DSH_ESTATE, "dsh_sketches_alloc first");
    if (src_p < c->p || src_p > kMaxP) return fail(c, DSH_EINVAL, "src_p=%d outside [%d,%d]", src_p, c->p, kMaxP);
    if (!slots_ok(first, n, c->n)) return fail(c, DSH_EINVAL, "slots [%llu,+%llu) out of range", (unsigned long long)first, (unsigned long long)n);
    return bind(c);
}

// One level of a union: the groups cptr/cdst over the rows of `src` (named through `mem`, or directly).  A group of more
// than K members is cut into chunks of K whose partial unions go to `part`; those rows are the next level's groups.
struct UnionLevel {
    std::vector<uint64_t> ptr;
    std::vector<uint32_t> dst;
};

int run_union(dsh_ctx *c, const uint64_t *gp, const uint32_t *members, uint64_t ng, uint8_t *d_out)
{
    const int p = c->p;
    const uint64_t blocks_per_row = std::max<uint64_t>(((uint64_t)1 << p) >> 12, 1);
    const uint64_t base = gp[0], total = gp[ng] - base;
    HIPCHK(c, c->derive.mem.ensure(std::max<uint64_t>(total, 1) * sizeof(uint32_t)));
    if (total) HIPCHK(c, hipMemcpyAsync(c->derive.mem.ptr, members + base, total * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    std::vector<uint64_t> cptr(ng + 1);
    std::vector<uint32_t> cdst(ng);
    for (uint64_t g = 0; g <= ng; ++g) cptr[g] = gp[g] - base;
    for (uint64_t g = 0; g < ng; ++g) cdst[g] = (uint32_t)g;
    std::vector<UnionLevel> keep;  // what the uploads of the levels read: alive until the stream is idle
    const uint8_t *src = c->regs;
    const uint32_t *mem = (const uint32_t *)c->derive.mem.ptr;
    for (int lvl = 0; !cdst.empty(); ++lvl) {
        // a workgroup streams its group's members one after the other: no group may hold more than a small share of the
        // launch's work (about 2048 workgroups run at a time), and none is cut below 64 members (a chunk costs a row of
        // scratch written and read again)
        const uint64_t cnt = cdst.size(), tot = cptr[cnt] - cptr[0];
        const uint64_t K = std::min<uint64_t>(std::max<uint64_t>(tot * blocks_per_row / 2048, 64), 1024);
        keep.emplace_back();
        UnionLevel &v = keep.back();
        std::vector<uint64_t> nptr(1, 0);
        std::vector<uint32_t> ndst;
        uint64_t srow = 0;
        for (uint64_t g = 0; g < cnt; ++g) {
            const uint64_t b = cptr[g], e = cptr[g + 1];
            if (e - b <= K) {
                v.ptr.push_back(b);
                v.dst.push_back(cdst[g]);
                continue;
            }
            for (uint64_t x = b; x < e; x += K) {
                v.ptr.push_back(x);
                v.dst.push_back(0x80000000u | (uint32_t)srow++);
            }
            nptr.push_back(srow);
            ndst.push_back(cdst[g]);
        }
        v.ptr.push_back(cptr[cnt]);
        if (srow >= 0x80000000ull) return fail(c, DSH_EINVAL, "too many members");
        const uint64_t nv = v.dst.size();
        DevBuf &part = c->derive.part[lvl & 1];
        HIPCHK(c, c->derive.ptr.ensure((nv + 1) * sizeof(uint64_t)));
        HIPCHK(c, c->derive.dst.ensure(nv * sizeof(uint32_t)));
        if (srow) HIPCHK(c, part.ensure(srow << p));
        HIPCHK(c, hipMemcpyAsync(c->derive.ptr.ptr, v.ptr.data(), (nv + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->derive.dst.ptr, v.dst.data(), nv * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, launch_union_groups(c->stream, src, p, (const uint64_t *)c->derive.ptr.ptr, mem, (const uint32_t *)c->derive.dst.ptr,
                                      nv, d_out, (uint8_t *)part.ptr));
        src = (const uint8_t *)part.ptr;
        mem = nullptr;
        cptr.swap(nptr);
        cdst.swap(ndst);
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
}

int check_union(dsh_ctx *c, const uint64_t *gp, const uint32_t *members, uint64_t ng)
{
    int rc = enter(c);
    if (rc) return rc;
    if (!ng) return DSH_OK;
    if (!gp) return DSH_EINVAL;
    if (ng >= 0x80000000ull) return fail(c, DSH_EINVAL, "too many groups");
    for (uint64_t g = 0; g < ng; ++g)
        if (gp[g + 1] < gp[g]) return fail(c, DSH_EINVAL, "group_ptr decreases at group %llu", (unsigned long long)g);
    if (gp[ng] > gp[0] && !members) return DSH_EINVAL;
    for (uint64_t x = gp[0]; x < gp[ng]; ++x)
        if (members[x] >= c->n)
            return fail(c, DSH_EINVAL, "members[%llu] = %u outside [0, %llu)", (unsigned long long)x, members[x], (unsigned long long)c->n);
    return DSH_OK;
}

}  // namespace

extern "C" {

int dsh_fold_device(dsh_ctx *c, uint64_t first, uint64_t n, int new_p, void *d_out)
{
    int rc = check_fold(c, first, n, new_p);
    if (rc || !n) return rc;
    if (!d_out) return DSH_EINVAL;
    if ((rc = err_begin(c))) return rc;
    HIPCHK(c, launch_fold(c->stream, c->regs + (first << c->p), n, c->p, new_p, first, (uint8_t *)d_out,
                          (unsigned long long *)c->derive.err.ptr));
    return err_end(c, c->p);
}

int dsh_fold(dsh_ctx *c, uint64_t first, uint64_t n, int new_p, uint8_t *out)
{
    int rc = check_fold(c, first, n, new_p);
    if (rc || !n) return rc;
    if (!out) return DSH_EINVAL;
    if ((rc = err_begin(c))) return rc;
    const uint64_t rows = std::min(chunk_rows(c, c->p), n);
    HIPCHK(c, c->derive.out.ensure(rows << new_p));
    for (uint64_t r0 = 0; r0 < n; r0 += rows) {
        const uint64_t cnt = std::min(rows, n - r0);
        if (launch_fold(c->stream, c->regs + ((first + r0) << c->p), cnt, c->p, new_p, first + r0, (uint8_t *)c->derive.out.ptr,
                        (unsigned long long *)c->derive.err.ptr) != hipSuccess ||
            hipMemcpyAsync(out + (r0 << new_p), c->derive.out.ptr, cnt << new_p, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
            return drain(c, fail(c, DSH_EIO, "fold of rows %llu.. failed", (unsigned long long)(first + r0)));
    }
    return err_end(c, c->p);
}

int dsh_upload_sketches_folded_device(dsh_ctx *c, const void *d_regs, int src_p, uint64_t first, uint64_t n)
{
    int rc = check_upload(c, src_p, first, n);
    if (rc || !n) return rc;
    if (!d_regs) return DSH_EINVAL;
    if ((rc = err_begin(c))) return rc;
    invalidate(c);
    HIPCHK(c, launch_fold(c->stream, (const uint8_t *)d_regs, n, src_p, c->p, first, (uint8_t *)c->regs_own.ptr + (first << c->p),
                          (unsigned long long *)c->derive.err.ptr));
    return err_end(c, src_p);
}

int dsh_upload_sketches_folded(dsh_ctx *c, const uint8_t *regs, int src_p, uint64_t first, uint64_t n)
{
    int rc = check_upload(c, src_p, first, n);
    if (rc || !n) return rc;
    if (!regs) return DSH_EINVAL;
    if ((rc = err_begin(c))) return rc;
    invalidate(c);
    const uint64_t rows = std::min(chunk_rows(c, src_p), n);
    HIPCHK(c, c->derive.stage.ensure(rows << src_p));
    for (uint64_t r0 = 0; r0 < n; r0 += rows) {
        // (the stream orders a chunk's fold before the next chunk's copy into the same scratch)
        const uint64_t cnt = std::min(rows, n - r0);
        if (hipMemcpyAsync(c->derive.stage.ptr, regs + (r0 << src_p), cnt << src_p, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
            launch_fold(c->stream, (const uint8_t *)c->derive.stage.ptr, cnt, src_p, c->p, first + r0,
                        (uint8_t *)c->regs_own.ptr + ((first + r0) << c->p), (unsigned long long *)c->derive.err.ptr) != hipSuccess)
            return drain(c, fail(c, DSH_EIO, "folded upload of rows %llu.. failed", (unsigned long long)(first + r0)));
    }
    return err_end(c, src_p);
}

int dsh_union_groups_device(dsh_ctx *c, const uint64_t *group_ptr, const uint32_t *members, uint64_t n_groups, void *d_out)
{
    int rc = check_union(c, group_ptr, members, n_groups);
    if (rc || !n_groups) return rc;
    if (!d_out) return DSH_EINVAL;
    if ((rc = run_union(c, group_ptr, members, n_groups, (uint8_t *)d_out))) return drain(c, rc);
    return DSH_OK;
}

int dsh_union_groups(dsh_ctx *c, const uint64_t *group_ptr, const uint32_t *members, uint64_t n_groups, uint8_t *out)
{
    int rc = check_union(c, group_ptr, members, n_groups);
    if (rc || !n_groups) return rc;
    if (!out) return DSH_EINVAL;
    HIPCHK(c, c->derive.out.ensure(n_groups << c->p));
    if ((rc = run_union(c, group_ptr, members, n_groups, (uint8_t *)c->derive.out.ptr))) return drain(c, rc);
    HIPCHK(c, hipMemcpyAsync(out, c->derive.out.ptr, n_groups << c->p, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return DSH_OK;
}

}  // extern "C"
