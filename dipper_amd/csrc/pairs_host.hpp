// Pairs within a distance threshold and their single-linkage clusters, restated on the host: plain C++, no HIP (include/dipper_hip.h,
// dpr_pairs_within_host).  A double loop over the strict lower triangle in (i, j) order and a union-find that always hangs the larger
// root under the smaller -- on purpose not the device's algorithm (row blocks, ballots and a scan, lock-free hooks; pairs.hip), which must
// reproduce it entry for entry and bit for bit.  Shared by the library (the host entry point, the summary of the device's labels), the
// command (the cluster ranks) and pairs_check.cpp (`make pairs_asan`).
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

namespace pairs {

// a threshold is a finite number >= 0 (NaN, an infinity and a negative number are refused)
inline bool threshold_ok(double t) { return t >= 0.0 && std::isfinite(t); }

inline int32_t find_root(const std::vector<int32_t>& parent, int32_t v)
{
    while (parent[(size_t)v] != v) v = parent[(size_t)v];
    return v;
}

// Every pair j < i with lower_rows[i (i - 1) / 2 + j] <= threshold in fp64 (NaN and +inf are never within it), ordered by i, then j.
// The first min(*count, cap) of them go to i[] / j[] / d[] (any of the three may be null when cap is 0); *count is the number found
// whatever cap is.  label[v] (n entries, may be null): the smallest index of v's connected component.  Returns 0, or -1 for a bad
// argument (nothing is written then).
inline int within_host(const double* lower_rows, int64_t n, double threshold, int32_t* i, int32_t* j, double* d, int64_t cap, int64_t* count,
                       int32_t* label)
{
    if (!lower_rows || n < 2 || n >= ((int64_t)1 << 31) || !threshold_ok(threshold) || cap < 0 || !count || (cap > 0 && (!i || !j || !d))) return -1;
    std::vector<int32_t> parent((size_t)n);
    for (int64_t v = 0; v < n; ++v) parent[(size_t)v] = (int32_t)v;
    int64_t k = 0;
    const double* row = lower_rows;
    for (int64_t a = 1; a < n; ++a) {
        row += a - 1;      // (row a starts a (a - 1) / 2 entries in)
        for (int64_t b = 0; b < a; ++b) {
            const double v = row[b];
            if (!(v <= threshold)) continue;
            if (k < cap) { i[k] = (int32_t)a; j[k] = (int32_t)b; d[k] = v; }
            ++k;
            const int32_t ra = find_root(parent, (int32_t)a), rb = find_root(parent, (int32_t)b);
            if (ra != rb) parent[(size_t)(ra > rb ? ra : rb)] = ra > rb ? rb : ra;
        }
    }
    *count = k;
    if (label)
        for (int64_t v = 0; v < n; ++v) label[(size_t)v] = find_root(parent, (int32_t)v);
    return 0;
}

// What the labels say: out[0] components, out[1] members of the largest, out[2] components of one member.  rank (n entries, may be
// null): the 1-based rank of every sequence's component, components ordered by their smallest member.  A label that is not the
// smallest index of a component -- label[v] > v, or label[label[v]] != label[v] -- returns -1.
inline int summarize(const int32_t* label, int64_t n, int64_t out[3], int32_t* rank)
{
    if (!label || n < 1 || !out) return -1;
    std::vector<int64_t> size((size_t)n, 0);
    for (int64_t v = 0; v < n; ++v) {
        const int32_t r = label[(size_t)v];
        if (r < 0 || r > v || label[(size_t)r] != r) return -1;
        ++size[(size_t)r];
    }
    std::vector<int32_t> rank_of((size_t)n, 0);
    int64_t comps = 0, largest = 0, single = 0;
    for (int64_t v = 0; v < n; ++v) {
        if (!size[(size_t)v]) continue;
        rank_of[(size_t)v] = (int32_t)++comps;
        if (size[(size_t)v] > largest) largest = size[(size_t)v];
        single += size[(size_t)v] == 1;
    }
    out[0] = comps; out[1] = largest; out[2] = single;
    if (rank)
        for (int64_t v = 0; v < n; ++v) rank[(size_t)v] = rank_of[(size_t)label[(size_t)v]];
    return 0;
}

}  // namespace pairs
