// Stand-alone driver of the host restatement of UPGMA / WPGMA (upgma_host.hpp), for builds with host sanitizers
// (`make upgma_asan`): noisy matrices, whole-number tie matrices, all-equal matrices, non-finite and negative-zero entries, bad
// arguments.  No GPU, no library.  Prints one line per case; exit status 0 unless a result is inconsistent.
#include "upgma_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

static uint64_t g_state = 1;
static double rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

int main()
{
    const int64_t sizes[] = { 2, 3, 4, 5, 8, 33, 120 };
    int bad = 0;
    for (int64_t n : sizes) {
        for (int linkage = 0; linkage < 2; ++linkage) {
            for (int shape = 0; shape < 5; ++shape) {      // noisy, whole-number ties, all equal, +inf and NaN, -0.0
                g_state = (uint64_t)(n * 131 + linkage * 17 + shape);
                std::vector<double> lower((size_t)(n * (n - 1) / 2));
                for (double& v : lower) v = shape == 1 ? 1.0 + std::floor(3.0 * rnd()) : shape == 2 ? 0.25 : 0.05 + rnd();
                if (shape == 3) { lower[0] = INFINITY; lower[lower.size() - 1] = NAN; lower[lower.size() / 2] = NAN; }
                if (shape == 4) { lower[0] = -0.0; lower[lower.size() - 1] = 0.0; }
                std::vector<int32_t> mx((size_t)(n - 1), -1), my((size_t)(n - 1), -1);
                std::vector<double> h((size_t)(n - 1), -1.0);
                const int rc = upgma::run_host(lower.data(), n, linkage, mx.data(), my.data(), h.data());
                // every entry is a slot pair of its iteration, the last one the root; finite input: heights of the order of the input
                bool ok = rc == 0;
                for (int64_t it = 0; ok && it < n - 1; ++it) ok = 0 <= mx[(size_t)it] && mx[(size_t)it] < my[(size_t)it] && my[(size_t)it] < n - it;
                ok = ok && mx[(size_t)(n - 2)] == 0 && my[(size_t)(n - 2)] == 1;
                const double top = shape == 1 ? 1.5 : 0.6;      // half the largest entry bounds every height of a finite input
                for (int64_t it = 0; ok && shape != 3 && it < n - 1; ++it) ok = h[(size_t)it] >= 0.0 && h[(size_t)it] <= top;
                if (shape == 3) ok = ok && h[(size_t)(n - 2)] != h[(size_t)(n - 2)];      // a NaN pair merges last and poisons the root
                std::printf("n %lld linkage %d shape %d: rc %d root height %.17g %s\n", (long long)n, linkage, shape, rc, h[(size_t)(n - 2)],
                            ok ? "ok" : "INCONSISTENT");
                bad += !ok;
                // bad arguments are refused before any memory is touched
                bad += upgma::run_host(lower.data(), 1, linkage, mx.data(), my.data(), h.data()) != -1;
                bad += upgma::run_host(lower.data(), n, 2, mx.data(), my.data(), h.data()) != -1;
                bad += upgma::run_host(nullptr, n, linkage, mx.data(), my.data(), h.data()) != -1;
                bad += upgma::run_host(lower.data(), n, linkage, mx.data(), nullptr, h.data()) != -1;
            }
        }
    }
    return bad ? 2 : 0;
}
