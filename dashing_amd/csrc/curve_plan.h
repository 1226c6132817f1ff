// curve_plan.h -- the host planning of dsh_union_curve* (curve.hip, kernels_curve.hip): into how many
// segments an order is cut, how many orders one batch holds, and the scratch a batch needs.  No HIP types here: curve.hip
// runs the planner for the device, libdashing_host.so for the CPU tests (host/plan_capi.cpp: dshh_curve_plan,
// tests/test_curve_plan.py).  A curve does not depend on the plan (the deltas are integers, the running maximum is
// associative): only these tests and the clock notice a changed cut.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace dsh {
namespace curve {

constexpr uint64_t kMinSegment = 64;          // members of a segment, unless forced: a segment costs a row of scratch written and read again
constexpr uint64_t kTargetWorkgroups = 2048;  // workgroups of a walk the planner aims at (about what runs at a time)
constexpr uint64_t kScanChunk = 128;          // steps per chunk of the two-level scan (k_curve_scan*)
constexpr uint64_t kMaxSteps = (uint64_t)1 << 31;  // steps (orders x len) of one batch: what the launches' grids take
constexpr uint64_t kDefaultScratch = (uint64_t)256 << 20;

struct Plan {
    uint64_t S = 1;          // members per segment (the last segment of an order may be shorter)
    uint64_t nseg = 0;       // segments per order: ceil(len / S)
    uint64_t nchunk = 0;     // scan chunks per order: ceil(len / kScanChunk)
    uint64_t batch = 1;      // orders per batch (the last batch may be smaller)
    uint64_t order_bytes = 0;  // delta + start rows + counters (+ chunk sums) of ONE order
    // segment s of an order holds the members [begin(s), begin(s + 1)) of it
    uint64_t begin(uint64_t s, uint64_t len) const { return std::min(s * S, len); }
    uint64_t scratch_bytes() const { return batch * order_bytes; }
};

inline uint64_t ceil_div(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// bytes of scratch one order needs when it is cut into nseg segments: int32 deltas [len][64], the counters the estimator
// reads [len][64] (uint16 up to p = 15, uint32 above), with more than one segment a start row per segment, with more than
// one scan chunk the chunks' sums
inline uint64_t order_scratch(uint64_t len, int p, uint64_t nseg)
{
    const uint64_t nchunk = ceil_div(len, kScanChunk);
    return len * 256 + len * 64 * (p <= 15 ? 2 : 4) + (nseg > 1 ? nseg << p : 0) + (nchunk > 1 ? nchunk * 256 : 0);
}

// S for `orders` orders walked in one launch: about kTargetWorkgroups workgroups of 4 KiB each, no segment below
// kMinSegment members (first choices, not measured: DESIGN.md 4.18)
inline uint64_t pick_segment(uint64_t orders, uint64_t len, int p)
{
    const uint64_t units = ceil_div(kTargetWorkgroups * 4096, (uint64_t)1 << p);  // (order, segment) units that make the target
    const uint64_t nseg = std::max<uint64_t>(ceil_div(units, std::max<uint64_t>(orders, 1)), 1);
    return std::min(std::max(ceil_div(len, nseg), kMinSegment), std::max<uint64_t>(len, 1));
}

// forced_S = 0: the planner's S.  The batch keeps batch * order_bytes within `budget` wherever one order fits it (else the
// batch is one order and the scratch grows to it).
inline Plan plan(uint64_t n_orders, uint64_t len, int p, uint64_t budget, uint64_t forced_S)
{
    Plan pl;
    uint64_t orders = std::max<uint64_t>(n_orders, 1);
    for (int round = 0; round < 2; ++round) {  // the batch decides S (workgroups of a launch), S the batch (start rows)
        pl.S = forced_S ? std::min(forced_S, std::max<uint64_t>(len, 1)) : pick_segment(orders, len, p);
        pl.nseg = ceil_div(len, pl.S);
        pl.nchunk = ceil_div(len, kScanChunk);
        pl.order_bytes = order_scratch(len, p, pl.nseg);
        uint64_t b = pl.order_bytes ? budget / pl.order_bytes : orders;
        if (len) b = std::min(b, kMaxSteps / len);
        if (pl.nseg) b = std::min(b, kMaxSteps / pl.nseg);
        b = std::min(std::max<uint64_t>(b, 1), orders);
        pl.batch = round ? std::min(pl.batch, b) : b;
        if (pl.batch == orders) break;
        orders = pl.batch;
    }
    return pl;
}

}  // namespace curve
}  // namespace dsh
