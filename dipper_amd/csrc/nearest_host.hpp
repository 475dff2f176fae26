// Each sequence's K nearest neighbours, restated on the host: plain C++, no HIP (include/dipper_hip.h, dpr_nearest_host).  A loop over
// the rows; a row's finite entries off the diagonal are gathered and std::partial_sort puts the first K in order under the comparator
// "smaller distance, then smaller column" -- on purpose not the device's algorithm (a running bound, ballots, a candidate buffer in LDS
// and selection by counting; nearest.hip), which must reproduce it entry for entry and bit for bit.  Shared by the library (the host
// entry point) and nearest_check.cpp (`make nearest_asan`).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace nearest {

constexpr int kNearestMaxK = 256;

// what pads a row with fewer than K neighbours: column -1 and this NaN, the same bits on the host and on the device
constexpr uint64_t kPadBits = 0x7ff8000000000000ull;
inline double pad_value()
{
    double v;
    const uint64_t b = kPadBits;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

struct Entry { double d; int32_t j; };

// a before b: the smaller distance in fp64 (-0.0 == +0.0: they tie), then the smaller column
inline bool before(const Entry& a, const Entry& b) { return a.d < b.d || (a.d == b.d && a.j < b.j); }

// lower_rows: the strict lower triangle row by row (row i holds i entries), read as a symmetric matrix.  For every row i the columns
// c != i with a finite entry, ordered by `before`; the first min(K, candidates) go to j[i K ..] / d[i K ..] (d: the entry's own bits), the
// rest of the K places holds -1 / pad_value(); cnt[i] = the places that are real.  Returns 0, or -1 for a bad argument (nothing is
// written then).
inline int nearest_host(const double* lower_rows, int64_t n, int K, int32_t* j, double* d, int32_t* cnt)
{
    if (!lower_rows || n < 2 || n >= ((int64_t)1 << 31) || K < 1 || K > kNearestMaxK || !j || !d || !cnt) return -1;
    std::vector<Entry> cand;
    cand.reserve((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        cand.clear();
        const double* row = lower_rows + i * (i - 1) / 2;
        for (int64_t c = 0; c < i; ++c)
            if (std::isfinite(row[c])) cand.push_back(Entry{ row[c], (int32_t)c });
        for (int64_t c = i + 1; c < n; ++c) {
            const double v = lower_rows[c * (c - 1) / 2 + i];
            if (std::isfinite(v)) cand.push_back(Entry{ v, (int32_t)c });
        }
        const size_t m = cand.size() < (size_t)K ? cand.size() : (size_t)K;
        std::partial_sort(cand.begin(), cand.begin() + (std::ptrdiff_t)m, cand.end(), before);
        for (size_t r = 0; r < (size_t)K; ++r) {
            j[(size_t)i * (size_t)K + r] = r < m ? cand[r].j : -1;
            d[(size_t)i * (size_t)K + r] = r < m ? cand[r].d : pad_value();
        }
        cnt[(size_t)i] = (int32_t)m;
    }
    return 0;
}

}  // namespace nearest
