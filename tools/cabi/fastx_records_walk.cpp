// fastx_records_walk.cpp -- the host arithmetic of dsh_sketch_fastx_records (csrc/sketch_plan.h: fastx_tail_records,
// fastx_line_start, fastx_record_offsets, then plan_records on their offsets; csrc/host/host.h: fastx_name_len) walked
// over random four-line FASTQ texts by a plain host program, so that it can run under the sanitizers -- it reads the
// first and last bytes of a file and walks backwards through it:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I dashing_amd/csrc
//     tools/cabi/fastx_records_walk.cpp -o tools/cabi/fastx_records_walk && tools/cabi/fastx_records_walk
// Every text lives in a heap block of exactly its length: one byte read before or behind it is reported.
// Exit status 0 and "ok": counts, header offsets and names equal a direct scan of the text; offsets are monotone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "host/host.h"
#include "sketch_plan.h"

using namespace dsh;

static void require(bool ok, const char *what, uint64_t a, uint64_t b)
{
    if (ok) return;
    std::fprintf(stderr, "fastx_records_walk: %s (%llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b);
    std::exit(1);
}

int main()
{
    std::mt19937_64 rng(12345);
    uint64_t checked = 0;
    for (int it = 0; it < 4000; ++it) {
        // nrec whole records, then one of the ways a text can end
        const int nrec = (int)(rng() % 5);
        std::string text;
        std::vector<uint64_t> hdr;  // the '@' of every record kseq returns
        for (int r = 0; r < nrec; ++r) {
            hdr.push_back(text.size());
            const size_t L = rng() % 7;
            text += "@n" + std::to_string(r) + (rng() & 1 ? " c" : "") + "\n" + std::string(L, 'A') + "\n+\n" + std::string(L, 'I') + "\n";
        }
        const int ending = (int)(rng() % 7);
        uint32_t markers = (uint32_t)nrec, end_line = 0;
        int64_t want = nrec;
        switch (ending) {
        case 0: break;
        case 1: if (!text.empty()) text.pop_back(), end_line = 3; break;            // no final newline
        case 2: hdr.push_back(text.size()), text += "@tail", ++want; break;        // inside a header line
        case 3: text += "@"; break;                                                // kseq's ordinary end
        case 4: hdr.push_back(text.size()), text += "@t\n", ++markers, ++want, end_line = 1; break;
        case 5: text += "@t\n\n+", ++markers, end_line = 2; break;                 // ends on the '+' line: no record
        case 6: hdr.push_back(text.size()), text += "@t\n\n+\n", ++markers, ++want, end_line = 3; break;
        }
        const uint64_t len = text.size();
        uint8_t *file = (uint8_t *)std::malloc(len ? len : 1);
        std::memcpy(file, text.data(), len);
        const int tail = fastx_tail_records(file, len, len && file[0] == '@' ? 1u : 0u, end_line);
        require((int64_t)markers + tail == want, "record count", it, (uint64_t)((int64_t)markers + tail));
        // the markers: the newline that ends every header line; decoded positions made up, increasing
        std::vector<uint64_t> rpos, dpos;
        for (uint64_t i = 0, line = 0; i < len; ++i)
            if (file[i] == '\n') {
                if ((line & 3) == 0) rpos.push_back(i), dpos.push_back(64 + 3 * rpos.size());
                ++line;
            }
        require(rpos.size() == markers, "markers", rpos.size(), markers);
        const uint64_t n = (uint64_t)want, used = std::min<uint64_t>(markers, n), end = 64 + 3 * (rpos.size() + 1);
        std::vector<uint64_t> off;
        fastx_record_offsets(dpos.data(), used, n, end, off);
        require(off.size() == n + 1 && off[n] == end, "offsets", off.size(), n);
        for (uint64_t r = 0; r < n; ++r) {
            require(off[r] <= off[r + 1], "offsets not monotone", r, off[r]);
            const uint64_t at = fastx_line_start(file, r < used ? rpos[r] : len - 1);
            require(at == hdr[r] && file[at] == '@', "header offset", at, hdr[r]);
            const size_t nl = dshh::fastx_name_len((const char *)file + at + 1, len - at - 1);
            require(nl >= 1 && at + 1 + nl <= len, "name", nl, len);
            ++checked;
        }
        std::vector<RecRun> runs;
        std::vector<RecSeg> segs;
        std::vector<uint32_t> zero;
        std::vector<SketchWork> work;
        if (n) require(plan_records(off.data(), (uint32_t)n, 5, 3, 10, runs, segs, zero, work), "plan_records", n, 0);
        std::free(file);
    }
    std::printf("ok (%llu records)\n", (unsigned long long)checked);
    return 0;
}
