// Stand-alone driver of nearest_host.hpp, for builds with host sanitizers (`make nearest_asan`): the K nearest neighbours of every row
// of random triangles with ties, NaN, +inf, -inf, -0.0 and negative entries, for K from 1 to beyond n; each answer checked against a
// second formulation (K times the smallest entry not taken yet, by a plain scan of the row); refused arguments.  No GPU, no library.
// Prints one line per case; exit status 0 unless a result is inconsistent.
#include "nearest_host.hpp"

#include <cstdio>

static uint64_t g_state = 1;
static double rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

static uint64_t bits(double v)
{
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

int main()
{
    const int64_t sizes[] = { 2, 3, 5, 17, 64, 65, 130, 300 };
    int bad = 0;
    for (int64_t n : sizes) {
        g_state = (uint64_t)(n * 7919);
        const int64_t cells = n * (n - 1) / 2;
        std::vector<double> lower((size_t)cells);
        for (double& v : lower) v = 0.05 * (double)(int)(rnd() * 20.0);      // twenty values: every row has runs of ties
        if (n >= 5) {
            lower[1] = NAN; lower[2] = INFINITY; lower[3] = -INFINITY; lower[(size_t)cells - 1] = NAN;
            lower[4] = -0.0; lower[5] = 0.0; lower[6] = -0.25;
        }
        if (n >= 17)
            for (int64_t c = 0; c < 7; ++c) lower[(size_t)(7 * 6 / 2 + c)] = c % 2 ? NAN : INFINITY;      // row 7: nothing finite below the diagonal
        auto at = [&](int64_t a, int64_t b) { return a > b ? lower[(size_t)(a * (a - 1) / 2 + b)] : lower[(size_t)(b * (b - 1) / 2 + a)]; };
        const int64_t Ks[] = { 1, 3, n > 2 ? n - 2 : 1, n - 1, n, 256 };
        for (int64_t k : Ks) {
            const int K = (int)(k < 256 ? k : 256);
            std::vector<int32_t> j((size_t)(n * K), -7), cnt((size_t)n, -7);
            std::vector<double> d((size_t)(n * K), -7.0);
            bool ok = nearest::nearest_host(lower.data(), n, K, j.data(), d.data(), cnt.data()) == 0;
            int64_t total = 0;
            for (int64_t i = 0; ok && i < n; ++i) {
                std::vector<char> taken((size_t)n, 0);
                int32_t m = 0;
                for (int r = 0; ok && r < K; ++r) {
                    int64_t best = -1;
                    for (int64_t c = 0; c < n; ++c) {
                        if (c == i || taken[(size_t)c] || !std::isfinite(at(i, c))) continue;
                        if (best < 0 || at(i, c) < at(i, best)) best = c;      // (the first of equal entries: the smaller column)
                    }
                    const size_t p = (size_t)(i * K + r);
                    if (best < 0) {
                        ok = j[p] == -1 && bits(d[p]) == nearest::kPadBits;
                    } else {
                        taken[(size_t)best] = 1;
                        ++m;
                        ok = j[p] == (int32_t)best && bits(d[p]) == bits(at(i, best));
                    }
                }
                ok = ok && cnt[(size_t)i] == m;
                total += m;
            }
            std::printf("n %lld K %d: neighbours %lld %s\n", (long long)n, K, (long long)total, ok ? "ok" : "INCONSISTENT");
            bad += !ok;
        }
        // refused: nothing is written
        std::vector<int32_t> j((size_t)n, -5), cnt((size_t)n, -5);
        std::vector<double> d((size_t)n, -5.0);
        bad += nearest::nearest_host(nullptr, n, 1, j.data(), d.data(), cnt.data()) != -1;
        bad += nearest::nearest_host(lower.data(), 1, 1, j.data(), d.data(), cnt.data()) != -1;
        bad += nearest::nearest_host(lower.data(), n, 0, j.data(), d.data(), cnt.data()) != -1;
        bad += nearest::nearest_host(lower.data(), n, 257, j.data(), d.data(), cnt.data()) != -1;
        bad += nearest::nearest_host(lower.data(), n, 1, nullptr, d.data(), cnt.data()) != -1;
        bad += nearest::nearest_host(lower.data(), n, 1, j.data(), nullptr, cnt.data()) != -1;
        bad += nearest::nearest_host(lower.data(), n, 1, j.data(), d.data(), nullptr) != -1;
        bad += j[0] != -5 || cnt[0] != -5 || d[0] != -5.0;
    }
    if (bad) std::printf("%d inconsistent\n", bad);
    return bad ? 2 : 0;
}
