// uf_dev.h -- the union-find of uf.h as the kernels reach it (kernels_cluster.hip, kernels_dbscan.hip): every access to
// parent[] is a relaxed agent-scope atomic (the XCDs have separate L2s; a plain load could also be served by a CU's L1 for
// ever), and an overrun of the step bound goes to the caller's one-word error buffer.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "uf.h"

namespace dsh {

struct UfDevice {
    static __device__ __forceinline__ uint32_t load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    static __device__ __forceinline__ uint32_t cas(uint32_t *p, uint32_t cmp, uint32_t val) { return atomicCAS(p, cmp, val); }
    static __device__ __forceinline__ void min(uint32_t *p, uint32_t val) { (void)atomicMin(p, val); }
};

// unite on the device: an overrun goes to the error word (first code wins nothing: any nonzero value fails the call)
__device__ __forceinline__ uint32_t cc_unite(uint32_t *parent, uint32_t a, uint32_t b, uint32_t cap, uint32_t *err)
{
    uint32_t why = 0;
    const uint32_t r = uf_unite<UfDevice>(parent, a, b, cap, &why);
    if (r == kUfOverrun) __hip_atomic_store(err, why, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return r;
}

}  // namespace dsh
