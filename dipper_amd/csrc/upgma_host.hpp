// UPGMA / WPGMA (average-linkage clustering; no reference counterpart).  Contract: include/dipper_hip.h above dpr_upgma_run.
// What the host restatement and the device loop share -- the order of values and the update arithmetic -- and the restatement
// itself (dpr_upgma_host): plain C++, no HIP, so that upgma_check.cpp can build it under host sanitizers.  The restatement is
// NAIVE on purpose: a full scan of the lower triangle per iteration, no cache of nearest neighbours; it is not the device's
// algorithm (upgma.hip), so that their agreement bit for bit means something.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#if defined(__HIPCC__)
#define UPGMA_HD __host__ __device__
#else
#define UPGMA_HD
#endif

namespace upgma {

// negative < zero (-0.0 as +0.0) < positive finite < +inf < NaN
UPGMA_HD inline uint64_t key(double v)
{
    if (v != v) return ~(uint64_t)0;
    uint64_t b;
    memcpy(&b, &v, sizeof b);
    if (b == ((uint64_t)1 << 63)) b = 0;
    return (b >> 63) ? ~b : (b | ((uint64_t)1 << 63));
}

// distance of the merged cluster to k; a = D[x][k], b = D[y][k], sx / sy the sizes before the merge
UPGMA_HD inline double merged(int linkage, double sx, double sy, double a, double b)
{
    return linkage == 0 ? (sx * a + sy * b) / (sx + sy) : 0.5 * (a + b);
}

// the whole loop over a square copy of the matrix; 0, or -1 for a bad argument.  rescans is not the host's to count.
inline int run_host(const double* lower_rows, int64_t n, int linkage, int32_t* merge_x, int32_t* merge_y, double* height)
{
    if (!lower_rows || n < 2 || n >= ((int64_t)1 << 24) || (linkage != 0 && linkage != 1) || !merge_x || !merge_y || !height) return -1;
    const size_t N = (size_t)n;
    std::vector<double> D(N * N, 0.0), s(N, 1.0);
    for (size_t i = 1, at = 0; i < N; ++i)
        for (size_t j = 0; j < i; ++j, ++at) D[i * N + j] = D[j * N + i] = lower_rows[at];
    for (int64_t it = 0; it < n - 1; ++it) {
        const size_t m = (size_t)(n - it);
        size_t x = 0, y = 1;
        uint64_t best = key(D[1 * N + 0]);
        for (size_t i = 0; i < m; ++i) {        // (key, i, j) ascending: i outer, j inner, strictly smaller keys only
            const double* row = &D[i * N];      // D[j][i] read as D[i][j]: the copy is symmetric bit for bit, and a row is contiguous
            for (size_t j = i + 1; j < m; ++j) {
                const uint64_t q = key(row[j]);
                if (q < best) { best = q; x = i; y = j; }
            }
        }
        const double d = D[y * N + x];
        merge_x[it] = (int32_t)x;
        merge_y[it] = (int32_t)y;
        height[it] = 0.5 * d;
        for (size_t k = 0; k < m; ++k) {
            if (k == x || k == y) continue;
            const double val = merged(linkage, s[x], s[y], D[x * N + k], D[y * N + k]);
            D[x * N + k] = D[k * N + x] = val;
        }
        s[x] = s[x] + s[y];
        const size_t last = m - 1;
        if (y != last) {
            for (size_t k = 0; k < m; ++k) D[y * N + k] = D[last * N + k];
            for (size_t k = 0; k < m; ++k) D[k * N + y] = D[k * N + last];
            s[y] = s[last];
        }
    }
    return 0;
}

}  // namespace upgma
