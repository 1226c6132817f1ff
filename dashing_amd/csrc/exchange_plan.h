// exchange_plan.h -- the host planning of dsh_exchange_* (exchange.hip): what every rank does under a row-set
// table (XMode), and the round schedule of dsh_exchange_collect_async -- which share of a source's buffer is message q,
// which part gates it, which rows the destination places behind round q, where everything lies in its buffers.  No HIP
// types here: exchange.hip runs the planner for the device, libdashing_host.so for the CPU tests (host/plan_capi.cpp:
// dshh_exchange_plan, tests/test_exchange_plan.py).  Both sides of a message run the same function, so the transport
// tests cannot notice a changed schedule: only these tests and the clock do.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "plan.h"

namespace dsh {
namespace xplan {

// what rank r does under dsh_exchange_*: the destination keeps its rows in place as ONE part; a short range, or any rank
// with extra segments, goes in row-sorted parts (every wanted segment key-ordered as one run, homogeneous tiles); a long
// range in parts of consecutive rows
struct XMode {
    bool rowsorted = false;
    uint64_t rb = 0, re = 0;      // the rank's main range
    std::vector<uint64_t> extra;  // its extra segments {b0, e0, ...}
    std::vector<uint64_t> cut;    // rowsorted: counts of wanted rows (wanted order); else row boundaries (range_parts)
    uint32_t kreq = 1;            // the number of parts asked of the part functions (what the compute call passes on)
    size_t nparts() const { return cut.empty() ? 0 : cut.size() - 1; }
    uint64_t span(uint64_t n) const { return plan::rowset_span(n, rb, re, extra); }
};

// Every rank's mode.  The parts are units of COMPLETION (a part's rows are final when k_finalize has passed them); what
// travels are MESSAGES: the q-th of `nparts` equal pieces of a source's buffer, sent as soon as the parts it overlaps are
// final (dsh_exchange_collect_async) -- the destination receives message q of every source in one round, and a round lasts
// as long as its largest message, so the messages of all sources are the same share of (about equal) spans.
// `fine_rank` >= 0: that rank (the caller, when its parts announce themselves from inside k_finalize: a part then costs a
// flag, not a launch) cuts its row-sorted rows as finely as they complete -- every tile row a part: a message waits for
// the part that holds its last value, and a coarse part that ends just short of a message's end would hold it back by a
// whole part.  Nobody else needs to know: the destination deals in messages and rows only.
inline std::vector<XMode> xmodes(uint64_t n, const plan::RowSets &rs, uint32_t nparts, int dst, int fine_rank = -1)
{
    std::vector<XMode> modes(rs.world);
    for (uint32_t r = 0; r < rs.world; ++r) {
        XMode &m = modes[r];
        rs.rank_rows(r, m.rb, m.re, m.extra);
        if (m.rb >= m.re) continue;
        if ((int)r == dst) {
            m.cut = {m.rb, m.re};
            continue;
        }
        m.rowsorted = !m.extra.empty() || plan::rowsorted_rule(n, m.rb, m.re, nparts);
        m.kreq = (m.rowsorted && (int)r == fine_rank) ? std::max<uint32_t>(nparts, kSigMaxParts) : nparts;
        if (m.rowsorted) plan::rowsorted_part_positions(n, m.rb, m.re, m.kreq, m.cut, &m.extra);
        else plan::range_parts(n, m.rb, m.re, nparts, m.cut);
    }
    return modes;
}

// message q of M of a buffer of `total` floats: [first, first + cnt)
inline void message_span(uint64_t total, size_t q, size_t M, uint64_t &first, uint64_t &cnt)
{
    first = (uint64_t)((unsigned __int128)total * q / M);
    cnt = (uint64_t)((unsigned __int128)total * (q + 1) / M) - first;
}

// the key order and the row offsets of a rank's row-sorted buffer (wanted rows: the extra segments, then the main range, each
// key-ordered as one run -- the main range as two where plan::rowsorted_split cuts it), from a host copy of the keys (every
// rank holds every sketch, the per-sketch pass is deterministic: the destination derives what the source used)
inline void rowsorted_tables(const uint32_t *keys, uint64_t n, const XMode &m, std::vector<uint32_t> &order, std::vector<uint64_t> &rowoff,
                             std::vector<uint32_t> &scratch)
{
    const uint64_t cnt = plan::rowset_rows(m.rb, m.re, m.extra);
    order.resize(cnt);
    std::vector<std::pair<uint64_t, uint64_t>> segs;  // the wanted order: extra segments first, then the main range
    plan::wanted_order(n, m.rb, m.re, &m.extra, segs, true);
    uint64_t at = 0;
    for (auto &sg : segs) {
        plan::sort_rows_by_key(keys, sg.first, sg.second, order.data() + at, scratch);
        at += sg.second - sg.first;
    }
    plan::rowsorted_offsets(n, order.data(), cnt, rowoff);
}

// where the parts of a rank end in its buffer: a row-sorted rank's at the offsets of its cut positions (rowoff_w: the
// offsets of its rows in the wanted order), a plain range's at its row boundaries; the destination computes relative to
// its first row, as one part that reaches to the end of its last segment.  Never decreasing.
inline std::vector<uint64_t> part_ends(uint64_t n, const XMode &m, const std::vector<uint64_t> &rowoff_w, bool is_dst)
{
    std::vector<uint64_t> part_end;
    for (size_t i = 0; i < m.nparts(); ++i) {
        uint64_t end;
        if (is_dst) end = plan::tri_span(n, m.rb, m.extra.empty() ? m.re : m.extra.back());
        else if (m.rowsorted) end = rowoff_w[m.cut[i + 1]];
        else end = plan::tri_span(n, m.rb, m.cut[i + 1]);
        part_end.push_back(std::max(end, part_end.empty() ? 0 : part_end.back()));
    }
    return part_end;
}

// THE gate of a message that ends at float x of the buffer (part_end not empty): the part that holds its last value --
// the first part that ends at or beyond x, the last part at most
inline size_t gate_part(const std::vector<uint64_t> &part_end, uint64_t x)
{
    return std::min((size_t)(std::lower_bound(part_end.begin(), part_end.end(), x) - part_end.begin()), part_end.size() - 1);
}

struct Msg { uint64_t first, cnt; };
// an entry of a round's placement launch (kernels.h: PlaceEnt) with the source's index in place of its device addresses
struct Ent { uint32_t src; uint64_t pos0; uint32_t row0, nrows; };
constexpr uint64_t kPlaceEntBytes = 40;  // sizeof(PlaceEnt)

// Everything dsh_exchange_collect_async decides before it touches a stream, for ONE calling rank.
struct Schedule {
    size_t M = 0;                  // rounds = messages per source
    int world = 0, dst = 0;
    std::vector<uint64_t> total;   // per source: the floats of its buffer (0: the destination, a rank without rows, and -- on a source -- the row-sorted others)
    std::vector<uint8_t> post;     // [q] the round is posted: a source's own message, or on the destination any source's, is not empty
    // the calling source: where its parts end in its buffer; [q] the last part the copy stream must have joined before
    // message q is posted (meaningful where the message is not empty)
    std::vector<uint64_t> part_end;
    std::vector<uint32_t> gate;
    // the destination: where the row-sorted sources are staged (floats) and where their tables lie in the upload (bytes:
    // per source rowoff then order, 16-byte aligned, behind them at ent_off the entries of all rounds) ...
    std::vector<uint64_t> stage_off, tab_off;
    uint64_t stage_total = 0, ent_off = 0, tab_bytes = 0;
    // ... and the placement launches: round q has the entries [round_ent[q], round_ent[q + 1]) and round_rows[q] rows
    std::vector<Ent> ents;
    std::vector<uint32_t> round_ent, round_rows;
    // message q of a source (of the sources whose total the caller knows)
    Msg msg(size_t q, int src) const
    {
        Msg m;
        message_span(src == dst ? 0 : total[(size_t)src], q, M, m.first, m.cnt);
        return m;
    }
};

// The exchange runs in M = nparts ROUNDS: message q of every source -- the q-th M-th of its buffer, whatever rows that
// is -- in one grouped ncclSend/ncclRecv.  A round lasts as long as its largest message, and the ranks' spans are
// about equal (dsh_balance_rowsets), so no link waits for another's longer message.  A source sends message q once
// the part that holds its last value is final (parts = units of completion, final in order); the destination's own rows
// are one part, computed in place, and gate nothing but the end of the call.
// modes: xmodes() of the table (with the calling rank as fine_rank where it cut finely).  rowoff[r]: the row offsets of the
// row-sorted rank r where the caller knows them -- a source knows its own (the layout's rowoff_w), the destination derives
// every source's (rowsorted_tables) -- else empty.
inline Schedule schedule(uint64_t n, const std::vector<XMode> &modes, uint32_t nparts, int dst, int rank,
                         const std::vector<std::vector<uint64_t>> &rowoff)
{
    Schedule S;
    const int world = (int)modes.size();
    const size_t M = nparts;
    const XMode &mine = modes[(size_t)rank];
    S.M = M, S.world = world, S.dst = dst;
    S.total.assign((size_t)world, 0), S.stage_off.assign((size_t)world, 0), S.tab_off.assign((size_t)world, 0);
    S.round_ent.assign(M + 1, 0), S.round_rows.assign(M, 0);
    for (int r = 0; r < world; ++r) {
        if (r == dst) continue;
        if (!modes[r].rowsorted) S.total[r] = plan::tri_span(n, modes[r].rb, modes[r].re);
        else if (!rowoff[r].empty()) S.total[r] = rowoff[r].back();
    }
    // row-sorted sources: the destination stages what it receives and puts the rows that are complete into place behind
    // every round
    for (int r = 0; r < world && rank == dst; ++r) {
        if (r == dst || !modes[r].rowsorted) continue;
        S.stage_off[r] = S.stage_total;
        S.stage_total += S.total[r];
        S.tab_off[r] = S.tab_bytes;
        S.tab_bytes += (rowoff[r].size() * sizeof(uint64_t) + (rowoff[r].size() - 1) * sizeof(uint32_t) + 15) & ~(uint64_t)15;
    }
    if (S.stage_total) {
        // behind the sources' tables: the entries of every round's placement launch (k_rows_place) -- the rows of a
        // source that lie completely inside its first q + 1 messages and did not inside its first q
        S.ent_off = S.tab_bytes;
        std::vector<uint64_t> rows_in((size_t)world, 0);
        for (size_t q = 0; q < M; ++q) {
            S.round_ent[q] = (uint32_t)S.ents.size();
            for (int src = 0; src < world; ++src) {
                if (src == dst || !modes[src].rowsorted) continue;
                const Msg m = S.msg(q, src);
                const std::vector<uint64_t> &ro = rowoff[src];  // ro[s] = start of the row at position s, ro.back() = total
                const uint64_t p1 = (uint64_t)(std::upper_bound(ro.begin(), ro.end(), m.first + m.cnt) - ro.begin()) - 1;
                const uint64_t p0 = rows_in[src];
                rows_in[src] = std::max(p0, p1);
                if (p1 <= p0) continue;
                S.ents.push_back(Ent{(uint32_t)src, p0, S.round_rows[q], (uint32_t)(p1 - p0)});
                S.round_rows[q] += (uint32_t)(p1 - p0);
            }
        }
        S.round_ent[M] = (uint32_t)S.ents.size();
        S.tab_bytes += S.ents.size() * kPlaceEntBytes;
    }
    // (source) where this rank's parts end in its buffer: message q waits for the part that holds its last value
    if (rank != dst) S.part_end = part_ends(n, mine, rowoff[rank], false);
    S.post.assign(M, 0), S.gate.assign(M, 0);
    for (size_t q = 0; q < M; ++q) {
        if (rank == dst) {
            for (int src = 0; src < world && !S.post[q]; ++src) S.post[q] = S.msg(q, src).cnt != 0;
        } else if (mine.nparts() && S.msg(q, rank).cnt) {
            S.post[q] = 1;
            S.gate[q] = (uint32_t)gate_part(S.part_end, S.msg(q, rank).first + S.msg(q, rank).cnt);
        }
    }
    return S;
}

}  // namespace xplan
}  // namespace dsh
