// vkey.h -- a float32 value as an order-preserving 32-bit integer, shared by the kernels that rank values with integer
// atomics (kernels_greedy.hip: the best representative; kernels_group.hip: the worst value of a group).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dsh {

// larger key = better value: the float's bits as an integer of the same order (-0.0 taken as +0.0 first, the bit-exact
// form of v + 0.0f: equal as float32 must mean equal here), complemented where a smaller value is better.  v is not NaN.
__device__ __forceinline__ uint32_t value_key32(float v, int descending)
{
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0u;
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if (!descending) u = ~u;
    return u;
}

// the value a key stands for (+0.0 for either zero)
__device__ __forceinline__ float value_of_key32(uint32_t u, int descending)
{
    if (!descending) u = ~u;
    u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
    return __uint_as_float(u);
}

}  // namespace dsh
