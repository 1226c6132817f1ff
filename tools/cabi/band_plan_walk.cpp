// band_plan_walk.cpp -- the band rule of csrc/plan.cpp (tri_band_end, rect_band_rows, greedy_old_band's use of the latter)
// walked over the grid of tests/test_band_plan.py by a plain host program, so that it can run under the sanitizers:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I dashing_amd/csrc
//     tools/cabi/band_plan_walk.cpp dashing_amd/csrc/plan.cpp -o tools/cabi/band_plan_walk && tools/cabi/band_plan_walk
// Exit status 0 and "ok": every walk covered its rows once, in order, inside both caps.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "plan.h"

using namespace dsh;
using namespace dsh::plan;

static void require(bool ok, const char *what, uint64_t a, uint64_t b, uint64_t c, uint64_t d)
{
    if (ok) return;
    std::fprintf(stderr, "band_plan_walk: %s (%llu, %llu, %llu, %llu)\n", what, (unsigned long long)a, (unsigned long long)b,
                 (unsigned long long)c, (unsigned long long)d);
    std::exit(1);
}

int main()
{
    const uint64_t ns[] = {0, 1, 2, 3, 129, 4097, 50000}, bytes[] = {4, 1000, 64 << 10, 1 << 30}, caps[] = {1, 7, 1 << 20};
    uint64_t nbands = 0;
    for (uint64_t n : ns)
        for (uint64_t by : bytes)
            for (uint64_t cap : caps) {
                const uint64_t floats = std::max<uint64_t>(by / 4, 1), max_rows = std::min<uint64_t>(cap, kBandMaxRows);
                const uint64_t ranges[4][2] = {{0, n}, {3, n / 2}, {n >= 2 ? n - 2 : 0, n}, {n / 3, n / 3}};
                for (const auto &rg : ranges)
                    for (uint64_t b0 = rg[0]; b0 < rg[1];) {
                        const uint64_t b1 = tri_band_end(n, b0, rg[1], floats, cap);
                        require(b1 > b0 && b1 <= rg[1], "band outside its range", n, b0, b1, rg[1]);
                        require(b1 - b0 <= max_rows, "too many rows", n, b0, b1, cap);
                        require(b1 - b0 == 1 || tri_span(n, b0, b1) <= floats, "too many values", n, b0, b1, floats);
                        require(b1 == rg[1] || b1 - b0 == max_rows || tri_span(n, b0, b1 + 1) > floats, "band ends early", n, b0, b1, floats);
                        b0 = b1;
                        ++nbands;
                    }
            }
    for (uint64_t ncols : {1, 5, 4097})
        for (uint64_t by : bytes) {
            const uint64_t floats = std::max<uint64_t>(by / 4, 1), rows = rect_band_rows(ncols, floats);
            require(rows >= 1 && rows <= kBandMaxRows && (rows == 1 || rows * ncols <= floats), "rectangle rows", ncols, by, rows, 0);
            require(rows == kBandMaxRows || (rows + 1) * ncols > floats, "rectangle band ends early", ncols, by, rows, 0);
            // the old rows of a greedy extension: every third slot a representative
            std::vector<uint32_t> labels(5000);
            for (uint32_t x = 0; x < labels.size(); ++x) labels[x] = x - x % 3;
            uint64_t b0 = 0, b1 = 0, last = 0;
            for (uint64_t from = 0; greedy_old_band(labels.data(), labels.size(), ncols, from, floats, b0, b1); from = b1) {
                require(b0 >= last && b1 > b0 && b1 - b0 <= rows && b1 <= labels.size(), "old band", ncols, by, b0, b1);
                last = b1;
                ++nbands;
            }
        }
    std::printf("ok: %llu bands\n", (unsigned long long)nbands);
    return 0;
}
