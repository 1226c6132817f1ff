// sketch_plan.h -- the sketch path's host planning: what the host fills for k_sketch, k_sketch_records and the FASTX
// decoder (kernels_sketch.hip, kernels_fastx.hip), and the pure functions that cut a call's offsets into those lists.
// No HIP types here: sketch.hip runs the planners for the device, libdashing_host.so for the CPU tests
// (host/plan_capi.cpp: dshh_sketch_plan, tests/test_sketch_plan.py), tools/cabi/sketch_plan_walk.cpp under the sanitizers.
// Also the arithmetic between the decoder's record index and plan_records (fastx_tail_records, fastx_line_start,
// fastx_record_offsets: tests/test_fastx_records_plan.py, tools/cabi/fastx_records_walk.cpp).
// Sketch results do not depend on the work list (the merge is a byte-wise max): only these tests notice a changed cut.
// The planners take offsets that are monotone and slots that fit 32 bits (sketch.hip: sketch_enter).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "consts.h"

namespace dsh {

struct SketchWork {
    uint64_t gbeg;   // absolute offset of the genome's first base in the device seq buffer
    uint64_t gend;   // one past its last base
    uint64_t start;  // absolute, 32-aligned offset of this workgroup's first base
    uint32_t nsub;   // number of 8192-base sub-chunks this workgroup walks
    uint32_t slot;   // row of the resident sketch matrix
};

// per-record sketches (dsh_sketch_records, k_sketch_records): a run is a stretch of whole, consecutive records that one
// workgroup owns -- their bases lie in [base, base + span) with span <= kRecRunSpan, their rows are slots
// [slot0, slot0 + nrec).  The records with at least one base are the run's segments: segs[seg0 + i] = {start of
// segment i relative to base, its slot relative to slot0}, starts strictly increasing, nseg <= kRecRunSegs.
constexpr uint32_t kRecRunSpan = 8192;  // bases of a run, counted from its 32-aligned base (256 lanes x 32)
constexpr uint32_t kRecRunSegs = 256;   // segments of a run (a k-mer's entry keeps its segment in 8 bits at p = 17)
constexpr uint32_t kRecRunRecs = 4096;  // records of a run, empty ones included
constexpr int kMaxPRecords = 17;        // largest p the records kernel takes (above: k_sketch's GLOBAL variant)
struct RecRun {
    uint64_t base;   // absolute, 32-aligned offset of the run's first base in the device seq buffer
    uint32_t seg0, nseg;
    uint32_t slot0, nrec;
    uint32_t span;   // end of the run's last base, relative to base
    uint32_t pad_;
};
struct RecSeg {  // (the kernel reads it as a uint2)
    uint32_t start, slot;
};

// FASTA text -> clean base stream on the device (kernels_fastx.hip).  A genome's raw file bytes lie at [off, off + rawlen)
// of the raw buffer (off 32-aligned) and are decoded to the same offset of the output buffer, the rest of the region up to
// region_end filled with 'N'; a chunk is what one workgroup takes (begin 32-aligned, len <= kFastxChunk).
constexpr uint32_t kFastxChunk = 16384;
struct FastxChunk {
    uint64_t begin;
    uint32_t len, genome;
};
struct FastxGenome {
    uint64_t off, rawlen, region_end;
    uint32_t chunk0, nchunks;
    uint32_t fmt, pad_;  // 0: FASTA (begins with '>'), 1: FASTQ in strict four-line records (begins with '@')
};

// sub-chunks (kSketchSub bases each) that k_sketch walks from the 32-aligned start of the genome [gb, ge)
inline uint64_t genome_subs(uint64_t gb, uint64_t ge) { return (ge - (gb & ~31ull) + kSketchSub - 1) / kSketchSub; }

// The sub-chunks a workgroup of k_sketch walks, for a call of total_subs sub-chunks in all.
// (Fewer sub-chunks per workgroup for SMALL calls -- a 46 MB batch of the streaming loader is 350 workgroups of 16 -- were
// tried in round 6 and lost: 2 sub-chunks = 2 785 workgroups took 147 us instead of 102, every workgroup ends by max-merging
// its 2^p registers into the same few rows of the matrix; profiles/rd6n, rd6o cli_kernel_stats.csv.)
// At BASELINE configs[1] size 16 is the optimum: 8 -> 8.43e11, 16 -> 8.59e11, 32 -> 8.31e11, 64 -> 8.2e11, 128 -> 8.3e11 bases/s
// (profiles/rd6p/sketch_subs_ab.jsonl).
// Large registers make the merge dear (a workgroup ends by max-merging its 2^p registers into the matrix) and leave few
// workgroups per CU: from p = 14 a workgroup walks more sub-chunks when the call is big enough to still give every CU
// several workgroups -- 300 x 5 Mbp, bases/s: p = 14 16 -> 64 sub-chunks 7.97e11 -> 8.17e11; p = 15 -> 128 6.38e11 ->
// 7.62e11 (256: 6.96e11); p = 16 4.63e11 -> 5.18e11; p = 17 3.35e11 -> 4.66e11; p = 13 stays at 16 (32: -3 %)
// (profiles/rd6af/sketch_subs_large_p.txt).
inline uint32_t subs_per_wg(int p, uint64_t total_subs)
{
    const uint32_t subs_cap = p <= 13 ? 16u : (p == 14 ? 64u : 128u);
    return (uint32_t)std::min<uint64_t>(subs_cap, std::max<uint64_t>(16, total_subs / 1024));
}

// the genome [gb, ge) of row `slot` as work items of up to `per` sub-chunks; none if it holds no k-mer
inline void cut_genome(uint64_t gb, uint64_t ge, uint32_t slot, int k, uint32_t per, std::vector<SketchWork> &work)
{
    if (ge - gb < (uint64_t)k) return;
    const uint64_t c0 = gb & ~31ull, nsub = genome_subs(gb, ge);
    for (uint64_t s = 0; s < nsub; s += per)
        work.push_back(SketchWork{gb, ge, c0 + s * kSketchSub, (uint32_t)std::min<uint64_t>(per, nsub - s), slot});
}

// dsh_sketch_batch*: genome g = [off[g], off[g + 1]) into row first_slot + g
inline void plan_genomes(const uint64_t *off, uint32_t n, uint64_t first_slot, int k, int p, std::vector<SketchWork> &work)
{
    uint64_t total_subs = 0;
    for (uint32_t g = 0; g < n; ++g) total_subs += genome_subs(off[g], off[g + 1]);
    const uint32_t per = subs_per_wg(p, total_subs);
    for (uint32_t g = 0; g < n; ++g) cut_genome(off[g], off[g + 1], (uint32_t)(first_slot + g), k, per, work);
}

// dsh_sketch_records*: the records split by length.  Those that fit kRecRunSpan bases from their 32-aligned base go to
// k_sketch_records in runs of whole consecutive records, cut greedily at the three caps (a workgroup each; the non-empty
// ones are the run's segments); a longer one is an ordinary genome for k_sketch (work) after its row is cleared (zero).
// false: p is above kMaxPRecords -- every record is a genome (work), and the caller clears all n rows at once
inline bool plan_records(const uint64_t *off, uint32_t n, uint64_t first_slot, int k, int p, std::vector<RecRun> &runs,
                         std::vector<RecSeg> &segs, std::vector<uint32_t> &zero, std::vector<SketchWork> &work)
{
    if (p > kMaxPRecords) {
        plan_genomes(off, n, first_slot, k, p, work);
        return false;
    }
    auto is_long = [&](uint32_t r) { return off[r + 1] - (off[r] & ~31ull) > kRecRunSpan; };
    uint64_t total_subs = 0;  // (of the long records: the others are not k_sketch's)
    for (uint32_t r = 0; r < n; ++r)
        if (is_long(r)) total_subs += genome_subs(off[r], off[r + 1]);
    const uint32_t per = subs_per_wg(p, total_subs);
    RecRun cur{};
    bool open = false;
    auto close = [&]() {
        if (open) runs.push_back(cur);
        open = false;
    };
    for (uint32_t r = 0; r < n; ++r) {
        const uint64_t b = off[r], e = off[r + 1];
        const uint32_t slot = (uint32_t)(first_slot + r);
        if (is_long(r)) {
            close();
            zero.push_back(slot);
            cut_genome(b, e, slot, k, per, work);
            continue;
        }
        if (open && (e - cur.base > kRecRunSpan || cur.nrec == kRecRunRecs || (e > b && cur.nseg == kRecRunSegs))) close();
        if (!open) {
            cur = RecRun{b & ~31ull, (uint32_t)segs.size(), 0, slot, 0, 0, 0};
            open = true;
        }
        if (e > b) {
            segs.push_back(RecSeg{(uint32_t)(b - cur.base), cur.nrec});
            ++cur.nseg;
            cur.span = (uint32_t)(e - cur.base);
        }
        ++cur.nrec;
    }
    close();
    return true;
}

// dsh_sketch_fastx_batch_async: the decoder's tables -- the genomes (raw file bytes of genome g at [off[g], off[g] + raw_len[g])
// of `raw`, its region up to off[g + 1]; the tables count from off[0]), then the chunks of their raw bytes.  Of `raw` only every
// genome's first byte is read.  Refusals: the code, and in *bad the genome it is about
enum { kFastxPlanOk = 0, kFastxPlanRegion = 1, kFastxPlanTooLarge = 2 };
inline int plan_fastx(const uint8_t *raw, const uint64_t *off, const uint64_t *raw_len, uint32_t n, std::vector<FastxGenome> &gen,
                      std::vector<FastxChunk> &chunks, uint32_t *bad)
{
    const uint64_t lo = n ? off[0] : 0;
    gen.resize(n);
    for (uint32_t g = 0; g < n; ++g) {
        const uint64_t b = off[g], e = off[g + 1];
        *bad = g;
        if (e < b || (b & 31) || raw_len[g] > e - b) return kFastxPlanRegion;
        gen[g].off = b - lo;
        gen[g].rawlen = raw_len[g];
        gen[g].fmt = (raw_len[g] && raw && raw[b] == '@') ? 1u : 0u;  // (the device checks that the rest keeps the promise)
        gen[g].pad_ = 0;
        gen[g].region_end = e - lo;
        gen[g].chunk0 = (uint32_t)chunks.size();
        for (uint64_t x = 0; x < raw_len[g]; x += kFastxChunk)
            chunks.push_back(FastxChunk{b - lo + x, (uint32_t)std::min<uint64_t>(kFastxChunk, raw_len[g] - x), g});
        gen[g].nchunks = (uint32_t)chunks.size() - gen[g].chunk0;
        if (chunks.size() > 0x7FFFFFFFull) return kFastxPlanTooLarge;
    }
    return kFastxPlanOk;
}

// dsh_sketch_fastx_records: kseq's records of an ACCEPTED file from the decoder's record markers (kernels.h: FastxRecIndex).
// Every marker is one record, but at the end of a FASTQ file (FASTA: the decoder itself leaves out a header character that
// is the file's last byte).  end_line is the index, modulo 4, of the line the file ends on; a file that ends with '\n' ends
// on a line nothing is on.  Returns the records to add to the markers:
//   +1  the file ends inside a header line of two bytes or more: kseq reads a name there and returns a last, empty record
//       (no newline ends that header, so it has no marker); "@" alone is kseq's ordinary end of file
//   -1  it ends on the '+' line with no newline behind it: kseq finds no quality string, an error -- its record is not
//       returned (the decoder accepted the file, so that record's sequence is empty)
inline int fastx_tail_records(const uint8_t *file, uint64_t len, uint32_t fmt, uint32_t end_line)
{
    if (fmt == 0 || len == 0 || file[len - 1] == '\n') return 0;
    if ((end_line & 3u) == 0) return (len >= 2 && file[len - 2] != '\n') ? 1 : 0;
    return (end_line & 3u) == 2 ? -1 : 0;
}

// the first byte of the line that holds file[pos] (a FASTQ marker is the newline that ENDS its header line)
inline uint64_t fastx_line_start(const uint8_t *file, uint64_t pos)
{
    while (pos && file[pos - 1] != '\n') --pos;
    return pos;
}

// plan_records' offsets for the n records of an accepted file: record r runs from its marker dpos[r] (the marker byte is
// invalid: it adds no k-mer) to the next one, the last to `end` -- the file's decoded end, not its region's: behind it lies
// padding, for FASTQ half the region.  Records without a marker (r >= markers: the +1 above) are empty, at `end`.
inline void fastx_record_offsets(const uint64_t *dpos, uint64_t markers, uint64_t n, uint64_t end, std::vector<uint64_t> &off)
{
    off.resize(n + 1);
    for (uint64_t r = 0; r < n; ++r) off[r] = r < markers ? dpos[r] : end;
    off[n] = end;
}

}  // namespace dsh
