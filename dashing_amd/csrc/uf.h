// uf.h -- the union-find of the threshold clusters (kernels_cluster.hip on the device, host/plan_capi.cpp for the CPU
// tests).  One source for both: the accesses to parent[] go through a policy A with
//   A::load(p)            the value at p
//   A::cas(p, cmp, val)   compare-and-swap, returns the value found
//   A::min(p, val)        p = min(p, val)
// (relaxed agent-scope atomics on the device, plain accesses in the sequential host build).
//
// parent[x] <= x AT ALL TIMES.  Only two kinds of write exist:
//   hook              cas(&parent[r], r, s) with s < r: a root goes under a smaller root
//   path shortening   min(&parent[x], g) with g an ancestor of x that was read before
// Both keep the invariant, so every path strictly decreases, no cycle can form, and the root a component ends with is its
// smallest member.  A stale read of parent[x] is an earlier value: x itself or an ancestor of x, a member of the same set.
// It costs a retry (the hook's cas then fails and returns the true parent), never a wrong merge.
//
// Every loop counts its steps against `cap` (the callers pass n + 1): uf_find follows at most n - 1 links, and uf_unite
// retries at most n - 1 times, because the larger of its two roots strictly decreases with every retry.  An overrun
// returns kUfOverrun; it is unreachable while the invariant holds and exists so that a bug ends with an error, not a hang.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DSH_UF_FN __host__ __device__ __forceinline__
#else
#define DSH_UF_FN inline
#endif

namespace dsh {

constexpr uint32_t kUfOverrun = 0xFFFFFFFFu;  // no node: the callers refuse n > 2^32 - 1
constexpr uint32_t kUfErrFind = 1, kUfErrHook = 2;  // what the callers store into their error word

// the root above x, shortening the path on the way (every node passed is re-pointed at its grandparent)
template <class A>
DSH_UF_FN uint32_t uf_find(uint32_t *parent, uint32_t x, uint32_t cap)
{
    uint32_t p = A::load(parent + x);
    for (uint32_t steps = 0; p != x; ++steps) {  // p < x
        if (steps >= cap) return kUfOverrun;
        const uint32_t g = A::load(parent + p);  // g <= p
        if (g != p) A::min(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// the sets of a and b become one.  Returns the root both are under afterwards as far as this call saw it (a member of
// the united set that was a root when read), kUfOverrun with *why set on a step-bound overrun.
template <class A>
DSH_UF_FN uint32_t uf_unite(uint32_t *parent, uint32_t a, uint32_t b, uint32_t cap, uint32_t *why)
{
    for (uint32_t tries = 0;; ++tries) {
        a = uf_find<A>(parent, a, cap);
        b = uf_find<A>(parent, b, cap);
        if (a == kUfOverrun || b == kUfOverrun) {
            *why = kUfErrFind;
            return kUfOverrun;
        }
        if (a == b) return a;
        if (a < b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t seen = A::cas(parent + a, a, b);  // hook: b < a
        if (seen == a) return b;
        if (tries >= cap) {
            *why = kUfErrHook;
            return kUfOverrun;
        }
        a = seen;  // a was hooked meanwhile: seen < a, and max(seen, b) < a
    }
}

// plain accesses: the sequential host build
struct UfPlain {
    static DSH_UF_FN uint32_t load(const uint32_t *p) { return *p; }
    static DSH_UF_FN uint32_t cas(uint32_t *p, uint32_t cmp, uint32_t val)
    {
        const uint32_t old = *p;
        if (old == cmp) *p = val;
        return old;
    }
    static DSH_UF_FN void min(uint32_t *p, uint32_t val)
    {
        if (val < *p) *p = val;
    }
};

}  // namespace dsh
