// comm.hip -- the communicator behind the multi-GPU C-ABI: librccl (dlopen'ed on first use), an RCCL communicator per
// context and its lifecycle (dsh_comm_*), the guarded wait of a stream that carries its traffic, the ONE poster of a grouped
// round of sends and receives (exchange.hip posts every message through it), the all-gather of register arrays after
// sharded sketching.
#include <dlfcn.h>

#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <cstdlib>
#include <cstring>

#include "ctx.h"

using namespace dsh;

namespace {

// RCCL, loaded on first use (std::call_once: the CLI's one-thread-per-device path may get here from several threads).
// The library must be the one built against the HIP runtime this file links to (the streams handed to it are ours):
// librccl.so.1 through this library's RUNPATH (/opt/rocm/lib), or DSH_RCCL_LIB.
// the entry points used, each under its name without the prefix (r->Send is ncclSend, with the type rccl.h declares)
#define DSH_RCCL_FNS(X) \
    X(GetUniqueId) X(CommInitRank) X(CommDestroy) X(CommAbort) X(GetVersion) X(GroupStart) X(GroupEnd) X(Send) X(Recv) X(AllGather) X(GetErrorString)
struct Rccl {
    void *h = nullptr;
#define DSH_RCCL_DECL(f) decltype(&nccl##f) f = nullptr;
    DSH_RCCL_FNS(DSH_RCCL_DECL)
    std::string err, path;
};

Rccl *rccl()
{
    static Rccl r;
    static std::once_flag once;
    std::call_once(once, [] {
        const char *names[3] = {std::getenv("DSH_RCCL_LIB"), "librccl.so.1", "/opt/rocm/lib/librccl.so.1"};
        for (const char *nm : names) {
            if (!nm || !*nm) continue;
            r.h = dlopen(nm, RTLD_NOW | RTLD_LOCAL);
            if (r.h) break;
            r.err = dlerror();
            if (nm == names[0]) return;  // an explicit DSH_RCCL_LIB that does not load is an error, not a hint
        }
        if (!r.h) return;
        auto sym = [&](const char *name) -> void * {
            void *p = dlsym(r.h, name);
            if (!p) r.err = std::string("librccl: missing symbol ") + name;
            return p;
        };
        bool all = true;  // (every symbol is asked for: `err` names the last one missing)
#define DSH_RCCL_LOAD(f) all &= (r.f = (decltype(r.f))sym("nccl" #f)) != nullptr;
        DSH_RCCL_FNS(DSH_RCCL_LOAD)
        if (!all) {
            dlclose(r.h);
            r.h = nullptr;
            return;
        }
        Dl_info di;
        if (dladdr((void *)r.GetUniqueId, &di) && di.dli_fname) r.path = di.dli_fname;
    });
    return &r;
}

#define NCCLCHK(c, expr)                                                                                   \
    do {                                                                                                   \
        ncclResult_t r_ = (expr);                                                                          \
        if (r_ != ncclSuccess) return fail((c), DSH_EIO, "%s: %s", #expr, rccl()->GetErrorString(r_));     \
    } while (0)

double env_seconds(const char *name, double dflt)
{
    const char *e = std::getenv(name);
    if (!e || !*e) return dflt;
    const double v = std::atof(e);
    return v > 0 ? v : dflt;
}

}  // namespace

namespace dsh {

// Wait for a stream that carries RCCL traffic, with a deadline: a peer that never posts its side of a grouped
// send/recv would otherwise block this rank for ever.  On expiry the communicator is aborted (its kernels leave the
// stream) and the call fails with a message; DSH_COMM_TIMEOUT_S (default 120) sets the deadline.
int sync_guarded(dsh_ctx *c, hipStream_t st, const char *what)
{
    if (!c->xch.comm || c->xch.world == 1) {
        HIPCHK(c, hipStreamSynchronize(st));
        return DSH_OK;
    }
    const double limit = env_seconds("DSH_COMM_TIMEOUT_S", 120.0);
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    for (;;) {
        const hipError_t q = hipStreamQuery(st);
        if (q == hipSuccess) return DSH_OK;
        if (q != hipErrorNotReady) return fail(c, DSH_EIO, "%s: %s", what, hipGetErrorString(q));
        if (++spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(50));
        if ((spins & 1023u) == 0 &&
            std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > limit) {
            (void)rccl()->CommAbort(c->xch.comm);
            c->xch.comm = nullptr;
            c->xch.rank = 0;
            c->xch.world = 1;
            return fail(c, DSH_EIO, "%s: the RCCL exchange did not complete within %.0f s (DSH_COMM_TIMEOUT_S): a peer "
                                    "is missing or stuck; the communicator was aborted", what, limit);
        }
    }
}

// bounds of `world` row ranges over n rows (dsh_balance_rows / dsh_partition_rows) and a destination rank: ONE check
// for every entry point that takes them
int validate_bounds(dsh_ctx *c, uint64_t n, const uint64_t *bounds, int world, int dst)
{
    if (!bounds) return fail(c, DSH_EINVAL, "bounds is NULL");
    if (dst < 0 || dst >= world) return fail(c, DSH_EINVAL, "bad destination rank %d (world %d)", dst, world);
    if (bounds[0] != 0 || bounds[world] != n) return fail(c, DSH_EINVAL, "bounds must run from 0 to n over the %d ranks", world);
    for (int r = 0; r < world; ++r)
        if (bounds[r] > bounds[r + 1]) return fail(c, DSH_EINVAL, "bounds not monotone at rank %d", r);
    return DSH_OK;
}

int comm_release(dsh_ctx *c)
{
    if (!c->xch.comm) return DSH_OK;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);  // dsh_collect_parts_async sends there
    const ncclResult_t e = rccl()->CommDestroy(c->xch.comm);
    c->xch.comm = nullptr;
    c->xch.rank = 0;
    c->xch.world = 1;
    return e == ncclSuccess ? DSH_OK : fail(c, DSH_EIO, "ncclCommDestroy: %s", rccl()->GetErrorString(e));
}

CommWho comm_who(const dsh_ctx *c) { return c->xch.comm ? CommWho{c->xch.world, c->xch.rank, true} : CommWho{1, 0, false}; }

int need_comm(dsh_ctx *c, bool alone_ok)
{
    return c->xch.comm || alone_ok ? DSH_OK : fail(c, DSH_ESTATE, "dsh_comm_init first");
}

// one grouped round: every operation of `ops`, in order, between ncclGroupStart and ncclGroupEnd on `st` (the group is
// closed behind a failed operation too).  A missing buffer counts as the operation's failure (ncclInvalidArgument)
int post_group(dsh_ctx *c, hipStream_t st, const GroupOp *ops, size_t nops)
{
    Rccl *r = rccl();
    NCCLCHK(c, r->GroupStart());
    ncclResult_t e = ncclSuccess;
    for (size_t x = 0; x < nops && e == ncclSuccess; ++x) {
        const GroupOp &o = ops[x];
        if (!o.ptr) e = ncclInvalidArgument;
        else if (o.send) e = r->Send(o.ptr, o.cnt, ncclFloat32, o.peer, c->xch.comm, st);
        else e = r->Recv(o.ptr, o.cnt, ncclFloat32, o.peer, c->xch.comm, st);
    }
    if (e != ncclSuccess) {
        (void)r->GroupEnd();
        return fail(c, DSH_EIO, "ncclSend/ncclRecv: %s", r->GetErrorString(e));
    }
    NCCLCHK(c, r->GroupEnd());
    return DSH_OK;
}

}  // namespace dsh

extern "C" {

/* ---- multi-GPU exchange through RCCL (one context per rank; ranks may be processes or threads) ------------------ */
int dsh_comm_available(void) { return rccl()->h ? DSH_OK : DSH_ENODEV; }

int dsh_comm_library(char *path_out, size_t cap, int *version_out)
{
    Rccl *r = rccl();
    if (!r->h) {
        if (path_out && cap) std::snprintf(path_out, cap, "%s", r->err.c_str());  // why it is not there
        return DSH_ENODEV;
    }
    if (path_out && cap) std::snprintf(path_out, cap, "%s", r->path.c_str());
    if (version_out) {
        int v = 0;
        if (r->GetVersion(&v) != ncclSuccess) v = 0;
        *version_out = v;
    }
    return DSH_OK;
}

int dsh_comm_unique_id(void *id_out)
{
    if (!id_out) return DSH_EINVAL;
    Rccl *r = rccl();
    if (!r->h) return DSH_ENODEV;
    ncclUniqueId id;
    if (r->GetUniqueId(&id) != ncclSuccess) return DSH_EIO;
    std::memcpy(id_out, &id, sizeof id);
    return DSH_OK;
}

int dsh_comm_init(dsh_ctx *c, const void *unique_id, int rank, int world)
{
    if (!c || !unique_id || world < 1 || rank < 0 || rank >= world) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    Rccl *r = rccl();
    if (!r->h) return fail(c, DSH_ENODEV, "RCCL is not available (%s)", r->err.c_str());
    if ((rc = comm_release(c))) return rc;  // re-initialisation: nothing of the old communicator is in flight any more
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof id);
    // ncclCommInitRank blocks until every rank has joined.  It runs on a helper thread so that a rank that never
    // arrives costs this one DSH_COMM_INIT_TIMEOUT_S (default 90 s) and an error, not a hang.  On expiry the helper
    // stays blocked inside RCCL and is left behind; the context works on without a communicator, and should the peers
    // arrive after all, the helper ABORTS the communicator it then gets (the peers would otherwise see a
    // successful init and stall until their exchange deadline).  All ranks must treat an init timeout as fatal.
    struct Shared {
        std::mutex mu;
        std::condition_variable cv;
        bool done = false;
        bool abandoned = false;
        ncclResult_t res = ncclSuccess;
        ncclComm_t comm = nullptr;
    };
    auto sh = std::make_shared<Shared>();
    const int device = c->device;
    auto init = r->CommInitRank;
    auto abort_ = r->CommAbort;
    std::thread([sh, device, init, abort_, world, id, rank] {
        ncclComm_t comm = nullptr;
        ncclResult_t res = hipSetDevice(device) == hipSuccess ? init(&comm, world, id, rank) : ncclUnhandledCudaError;
        bool orphan = false;
        {
            std::lock_guard<std::mutex> lk(sh->mu);
            sh->res = res;
            sh->comm = comm;
            sh->done = true;
            orphan = sh->abandoned;
            sh->cv.notify_all();
        }
        if (orphan && res == ncclSuccess && comm) (void)abort_(comm);  // nobody will ever use or destroy it
    }).detach();
    const double limit = env_seconds("DSH_COMM_INIT_TIMEOUT_S", 90.0);
    {
        std::unique_lock<std::mutex> lk(sh->mu);
        if (!sh->cv.wait_for(lk, std::chrono::duration<double>(limit), [&] { return sh->done; })) {
            sh->abandoned = true;
            return fail(c, DSH_EIO, "ncclCommInitRank(rank %d of %d) did not return within %.0f s (DSH_COMM_INIT_TIMEOUT_S): "
                                    "not every rank joined", rank, world, limit);
        }
        if (sh->res != ncclSuccess) return fail(c, DSH_EIO, "ncclCommInitRank: %s", r->GetErrorString(sh->res));
        c->xch.comm = sh->comm;
    }
    c->xch.rank = rank;
    c->xch.world = world;
    return DSH_OK;
}

int dsh_comm_destroy(dsh_ctx *c)
{
    if (!c) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    return comm_release(c);
}

int dsh_comm_rank(const dsh_ctx *c, int *rank, int *world)
{
    if (!c) return DSH_EINVAL;
    if (rank) *rank = c->xch.rank;
    if (world) *world = c->xch.comm ? c->xch.world : 1;
    return c->xch.comm ? DSH_OK : DSH_ESTATE;
}

int dsh_comm_wait(dsh_ctx *c)
{
    if (!c) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    if ((rc = sync_guarded(c, c->stream, "dsh_comm_wait (ctx stream)"))) return rc;
    return sync_guarded(c, c->copy_stream, "dsh_comm_wait (copy stream)");
}

int dsh_allgather_device(dsh_ctx *c, const void *d_send, uint64_t bytes_per_rank, void *d_recv)
{
    if (!c || (bytes_per_rank && (!d_send || !d_recv))) return DSH_EINVAL;
    int rc = bind(c);
    if (rc) return rc;
    if (!c->xch.comm) return fail(c, DSH_ESTATE, "dsh_comm_init first");
    if (bytes_per_rank) NCCLCHK(c, rccl()->AllGather(d_send, d_recv, bytes_per_rank, ncclUint8, c->xch.comm, c->stream));
    return sync_guarded(c, c->stream, "dsh_allgather_device");
}

}  // extern "C"
