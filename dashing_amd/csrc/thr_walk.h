// thr_walk.h -- how the kernels that consume a band of dense values walk its rows (ThrRows, kernels.h; the host side is
// bands.h).  Row r of the band buffer is either a row of the packed triangle (collection row i = row0 + r, n - 1 - i values,
// columns i + 1 ..., starting at ANY 4-byte offset of the buffer) or a row of a rectangle (ncols values, columns col0 ...).
// A row is cut into chunks of kThrChunk values; block (r, y) of thr_grid holds four waves, wave w the chunk 4 y + w of band
// row r, which it walks front to back kThrStep values per step: one float4 per lane.  Device code only: plain inlined
// functions, which leave the kernels' register counts where the hand-written walks had them.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace dsh {

constexpr uint32_t kThrStep = 256;  // values a wave takes per step: one float4 per lane

__device__ __forceinline__ bool thr_pass(float v, float t, int descending) { return descending ? v >= t : v <= t; }  // NaN: neither

// first value of row r of a band of triangle rows whose first row holds `first` values: the sum of (first - t) over t < r
// (r = 0: the product is 0)
__device__ __forceinline__ uint64_t band_rowoff(uint64_t first, uint64_t r) { return r * first - r * (r - 1) / 2; }

struct ThrRow {
    uint64_t rowoff;   // first value of the row in the band buffer
    uint64_t len;      // values of the row
    uint32_t colbase;  // column of the row's first value
};

// row r of a band of TRIANGLE rows (!g.rect, which the launchers of the kernels that call this see to): the collection row
// is g.row0 + r = colbase - 1
__device__ __forceinline__ ThrRow thr_tri_row(const ThrRows &g, uint64_t r)
{
    const uint64_t i = g.row0 + r;
    ThrRow c;
    c.len = g.n - 1 - i;
    c.rowoff = band_rowoff(g.n - 1 - g.row0, r);  // (row0 < n)
    c.colbase = (uint32_t)(i + 1);
    return c;
}

// row r of the rows of a RECTANGLE (g.rect)
__device__ __forceinline__ ThrRow thr_rect_row(const ThrRows &g, uint64_t r)
{
    ThrRow c;
    c.len = g.ncols;
    c.rowoff = r * g.ncols;
    c.colbase = (uint32_t)g.col0;
    return c;
}

__device__ __forceinline__ ThrRow thr_row(const ThrRows &g, uint64_t r) { return g.rect ? thr_rect_row(g, r) : thr_tri_row(g, r); }

// chunk ch starts inside a row of len values
__device__ __forceinline__ bool thr_chunk_inside(uint64_t len, uint32_t ch) { return (uint64_t)ch * kThrChunk < len; }

// chunk ch of a row: its values are [begin, end) of the band buffer; false: the chunk lies behind the row's end
__device__ __forceinline__ bool thr_chunk(ThrRow row, uint32_t ch, uint64_t &begin, uint64_t &end)
{
    const uint64_t cb = (uint64_t)ch * kThrChunk;
    begin = row.rowoff + cb;
    end = row.rowoff + (row.len - cb < kThrChunk ? row.len : cb + kThrChunk);  // (read only where cb < len)
    return thr_chunk_inside(row.len, ch);
}

// where a lane starts in the chunk [begin, end): begin rounded DOWN to a multiple of 4, so that every full group of four is
// one aligned 16-byte load (the buffer's base is 256-byte aligned); then idx += kThrStep while idx < end
__device__ __forceinline__ uint64_t thr_first(uint64_t begin, uint32_t lane) { return (begin & ~(uint64_t)3) + 4 * lane; }

// The lane's four values idx .. idx + 3 of the chunk [begin, end) and their hit flags (thr_pass; bit c: v[c]): one aligned
// float4 load where all four lie inside, value by value where begin or end cuts the group (outside: v[c] = 0, no flag).
__device__ __forceinline__ uint32_t thr_flags(const float *__restrict__ vals, uint64_t idx, uint64_t begin, uint64_t end, float t,
                                              int descending, float v[4])
{
    uint32_t m = 0;
    if (idx >= begin && idx + 4 <= end) {
        const float4 q = *reinterpret_cast<const float4 *>(vals + idx);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
#pragma unroll
        for (int c = 0; c < 4; ++c) m |= (thr_pass(v[c], t, descending) ? 1u : 0u) << c;
    } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            v[c] = 0.f;
            if (idx + c >= begin && idx + c < end) {
                v[c] = vals[idx + c];
                m |= (thr_pass(v[c], t, descending) ? 1u : 0u) << c;
            }
        }
    }
    return m;
}

}  // namespace dsh
