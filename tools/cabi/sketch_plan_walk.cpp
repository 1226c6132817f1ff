// sketch_plan_walk.cpp -- the sketch path's planners (csrc/sketch_plan.h: plan_genomes, plan_records, plan_fastx) walked
// over the grid of tests/test_sketch_plan.py by a plain host program, so that they can run under the sanitizers -- they are
// full of 64-to-32-bit narrowing and unsigned differences:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I dashing_amd/csrc
//     tools/cabi/sketch_plan_walk.cpp -o tools/cabi/sketch_plan_walk && tools/cabi/sketch_plan_walk
// Exit status 0 and "ok": every list covered its input once, in order, inside its caps, and no narrowing lost a bit.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "sketch_plan.h"

using namespace dsh;

static void require(bool ok, const char *what, uint64_t a, uint64_t b, uint64_t c, uint64_t d)
{
    if (ok) return;
    std::fprintf(stderr, "sketch_plan_walk: %s (%llu, %llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b,
                 (unsigned long long)c, (unsigned long long)d);
    std::exit(1);
}

static std::vector<uint64_t> offsets(const std::vector<uint64_t> &lens, uint64_t lead)
{
    std::vector<uint64_t> off(lens.size() + 1, lead);
    for (size_t i = 0; i < lens.size(); ++i) off[i + 1] = off[i] + lens[i];
    return off;
}

// the items of [b, e) for `slot`, from work[at] on: consecutive, `per` sub-chunks each but the last
static void walk_items(const std::vector<SketchWork> &work, size_t &at, uint64_t b, uint64_t e, uint64_t slot, int k, uint32_t per)
{
    if (e - b < (uint64_t)k) return;
    for (uint64_t pos = b & ~31ull;;) {
        require(at < work.size(), "items missing", b, e, slot, at);
        const SketchWork &w = work[at++];
        require(w.gbeg == b && w.gend == e && w.slot == slot && w.start == pos, "item of another genome or place", b, e, w.start, pos);
        require(w.nsub >= 1 && w.nsub <= per, "item size", b, e, w.nsub, per);
        pos += (uint64_t)w.nsub * kSketchSub;
        if (pos >= e) {
            require(pos - kSketchSub < e, "a sub-chunk behind the end", b, e, pos, 0);
            return;
        }
        require(w.nsub == per, "a short item that is not the last", b, e, w.nsub, per);
    }
}

static uint64_t walk_genomes(const std::vector<uint64_t> &off, uint64_t first, int k, int p)
{
    const uint32_t n = (uint32_t)(off.size() - 1);
    std::vector<SketchWork> work;
    plan_genomes(off.data(), n, first, k, p, work);
    uint64_t total = 0;
    for (uint32_t g = 0; g < n; ++g) total += genome_subs(off[g], off[g + 1]);
    size_t at = 0;
    for (uint32_t g = 0; g < n; ++g) walk_items(work, at, off[g], off[g + 1], first + g, k, subs_per_wg(p, total));
    require(at == work.size(), "items nobody asked for", at, work.size(), k, p);
    return work.size();
}

static uint64_t walk_records(const std::vector<uint64_t> &off, uint64_t first, int k, int p)
{
    const uint32_t n = (uint32_t)(off.size() - 1);
    std::vector<RecRun> runs;
    std::vector<RecSeg> segs;
    std::vector<uint32_t> zero;
    std::vector<SketchWork> work;
    if (!plan_records(off.data(), n, first, k, p, runs, segs, zero, work)) {
        require(p > kMaxPRecords && runs.empty() && segs.empty() && zero.empty(), "the genome way below its p", p, runs.size(), 0, 0);
        return walk_genomes(off, first, k, p);
    }
    auto is_long = [&](uint32_t r) { return off[r + 1] - (off[r] & ~31ull) > kRecRunSpan; };
    uint64_t total = 0;
    for (uint32_t r = 0; r < n; ++r)
        if (is_long(r)) total += genome_subs(off[r], off[r + 1]);
    size_t at = 0, nz = 0, ns = 0;
    uint32_t r = 0;
    auto long_record = [&](uint32_t q) {  // its row is cleared, and it is cut like a genome
        require(nz < zero.size() && zero[nz] == first + q, "a long record's row is not cleared", q, nz, 0, 0);
        ++nz;
        walk_items(work, at, off[q], off[q + 1], first + q, k, subs_per_wg(p, total));
    };
    for (const RecRun &u : runs) {
        for (; r < n && is_long(r); ++r) long_record(r);
        require(r < n && u.slot0 == first + r && u.base == (off[r] & ~31ull) && u.seg0 == ns, "run start", r, u.slot0, u.base, u.seg0);
        require(u.nrec >= 1 && u.nrec <= kRecRunRecs && u.nseg <= kRecRunSegs && u.span <= kRecRunSpan && r + u.nrec <= n, "run caps", u.nrec, u.nseg, u.span, r);
        uint32_t nseg = 0;
        for (uint32_t q = r; q < r + u.nrec; ++q) {
            require(!is_long(q) && off[q + 1] - u.base <= kRecRunSpan, "a record that does not fit its run", q, u.base, off[q + 1], 0);
            if (off[q + 1] == off[q]) continue;
            require(ns < segs.size() && segs[ns].start == off[q] - u.base && segs[ns].slot == q - r, "segment", q, ns, u.base, 0);
            require(nseg == 0 || segs[ns].start > segs[ns - 1].start, "segment starts do not increase", q, ns, 0, 0);
            require(u.span >= off[q + 1] - u.base, "span", q, u.span, 0, 0);
            ++ns, ++nseg;
        }
        require(nseg == u.nseg, "segment count", r, nseg, u.nseg, 0);
        r += u.nrec;
        if (r < n && !is_long(r))
            require(off[r + 1] - u.base > kRecRunSpan || u.nrec == kRecRunRecs || (off[r + 1] > off[r] && u.nseg == kRecRunSegs), "run ends early", r, u.nrec, u.nseg, u.span);
    }
    for (; r < n; ++r) {
        require(is_long(r), "a record in no run", r, n, 0, 0);
        long_record(r);
    }
    require(at == work.size() && nz == zero.size() && ns == segs.size(), "entries nobody asked for", at, nz, ns, 0);
    return runs.size() + work.size();
}

static uint64_t walk_fastx(const std::vector<uint64_t> &off, const std::vector<uint64_t> &raw_len, const std::vector<uint8_t> &raw)
{
    const uint32_t n = (uint32_t)raw_len.size();
    std::vector<FastxGenome> gen;
    std::vector<FastxChunk> chunks;
    uint32_t bad = 0;
    require(plan_fastx(raw.data(), off.data(), raw_len.data(), n, gen, chunks, &bad) == kFastxPlanOk, "refused", bad, 0, 0, 0);
    size_t at = 0;
    for (uint32_t g = 0; g < n; ++g) {
        const uint64_t b = off[g] - off[0];
        require(gen[g].off == b && gen[g].rawlen == raw_len[g] && gen[g].region_end == off[g + 1] - off[0] && gen[g].chunk0 == at, "genome", g, b, at, 0);
        require(gen[g].fmt == (raw_len[g] && raw[off[g]] == '@' ? 1u : 0u) && gen[g].pad_ == 0, "format", g, gen[g].fmt, 0, 0);
        for (uint64_t x = 0; x < raw_len[g]; x += kFastxChunk, ++at)
            require(at < chunks.size() && chunks[at].begin == b + x && chunks[at].genome == g && chunks[at].len == std::min<uint64_t>(kFastxChunk, raw_len[g] - x), "chunk", g, x, at, 0);
        require(gen[g].nchunks == at - gen[g].chunk0, "chunk count", g, at, 0, 0);
    }
    require(at == chunks.size(), "chunks nobody asked for", at, chunks.size(), 0, 0);
    // refusals name the genome
    if (n > 2) {
        std::vector<uint64_t> o2 = off, l2 = raw_len;
        o2[2] += 1;
        require(plan_fastx(raw.data(), o2.data(), l2.data(), n, gen, chunks, &bad) == kFastxPlanRegion && bad == 2, "an unaligned region passed", bad, 0, 0, 0);
        l2[1] = off[2] - off[1] + 1;
        require(plan_fastx(raw.data(), off.data(), l2.data(), n, gen, chunks, &bad) == kFastxPlanRegion && bad == 1, "raw bytes beyond the region passed", bad, 0, 0, 0);
    }
    return chunks.size();
}

int main()
{
    std::mt19937_64 rng(1);
    auto upto = [&](uint64_t m) { return (uint64_t)(rng() % (m + 1)); };
    uint64_t entries = 0;
    const int ps[] = {4, 10, 13, 14, 15, 17, 18, 24}, ks[] = {1, 31, 32};
    // the rule at its thresholds, from a few huge offsets (the planners never read the bases)
    for (int p : ps)
        for (uint64_t edge : {17u * 1024, 64u * 1024, 128u * 1024})
            for (uint64_t total = edge - 1; total <= edge + 1; ++total) {
                const std::vector<uint64_t> off = offsets({total / 3 * kSketchSub, 5ull * kSketchSub, (total - total / 3 - 6) * kSketchSub, 30}, 0);
                entries += walk_genomes(off, 3, 31, p) + walk_records(off, 3, 31, p);
            }
    // slots at the top of 32 bits, offsets beyond them
    entries += walk_genomes(offsets({100, 0, 20000, 8193}, (1ull << 40) + 13), 0xFFFFFFFFull - 4, 31, 14);
    entries += walk_records(offsets({100, 0, 20000, 8193}, (1ull << 40) + 13), 0xFFFFFFFFull - 4, 31, 14);
    // edge lengths on every lane offset; random lengths
    const std::vector<uint64_t> edge = {0, 1, 30, 31, 32, 33, 5, 4, 6, 20, 21, 22, 150, 1000, 8191, 8192, 8193, 0, 0, 2, 64, 65, 63, 7000, 1200,
                                        16 * 8192, 16 * 8192 + 5, 17 * 8192, 33 * 8192 + 123};
    for (uint64_t lead = 0; lead < 33; ++lead)
        for (int p : ps)
            for (int k : ks) entries += walk_genomes(offsets(edge, lead), 2, k, p) + walk_records(offsets(edge, lead), 2, k, p);
    for (int it = 0; it < 200; ++it) {
        std::vector<uint64_t> lens(1 + upto(400));
        for (uint64_t &x : lens) x = upto(3) == 0 ? 0 : upto(1ull << upto(18));
        const int p = ps[upto(7)], k = 1 + (int)upto(31);
        entries += walk_genomes(offsets(lens, upto(100)), upto(5), k, p) + walk_records(offsets(lens, upto(100)), upto(5), k, p);
    }
    // the caps of a run: 300 one-base records (segments), 10 000 mostly empty ones (records), 8191 / 8192 / 8193 bases at lane offsets
    entries += walk_records(offsets(std::vector<uint64_t>(300, 1), 7), 0, 1, 10);
    std::vector<uint64_t> sparse(10000, 0);
    for (size_t i = 0; i < sparse.size(); i += 97) sparse[i] = 1 + upto(58);
    entries += walk_records(offsets(sparse, 0), 0, 21, 10);
    for (uint64_t o : {0, 1, 31})
        for (uint64_t L : {8191, 8192, 8193}) entries += walk_records(offsets({L}, 64 + o), 4, 31, 10);
    // FASTX tables
    for (int it = 0; it < 20; ++it) {
        const uint32_t n = 1 + (uint32_t)upto(40);
        std::vector<uint64_t> raw_len(n), region(n);
        for (uint32_t g = 0; g < n; ++g) {
            raw_len[g] = upto(4) == 0 ? upto(2) * kFastxChunk : upto(5 * kFastxChunk);
            region[g] = (raw_len[g] + upto(99) + 31) / 32 * 32;
        }
        const std::vector<uint64_t> off = offsets(region, 64);
        std::vector<uint8_t> raw(off[n] + 1, 'A');
        for (uint32_t g = 0; g < n; ++g) raw[off[g]] = ">@;"[upto(2)];
        entries += walk_fastx(off, raw_len, raw);
    }
    std::printf("ok: %llu entries\n", (unsigned long long)entries);
    return 0;
}
