// Stand-alone driver of the host restatement of the BME SPR search (bme_host.hpp), for builds with host sanitizers
// (`make bme_spr_asan`): random noisy matrices with a caterpillar and a random merge log, non-finite entries, every (d, w) of
// the single-move hook on the small sizes, bad logs and bad children tables.  No GPU, no library.  Prints one line per case;
// exit status 0 unless a result is inconsistent.
#include "bme_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace dpr::bme;

static uint64_t g_state = 1;
static double rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

int main(int argc, char** argv)
{
    const int64_t sizes[] = { 3, 4, 5, 8, 33, 120 };
    int bad = 0;
    for (int64_t n : sizes) {
        for (int shape = 0; shape < 2; ++shape) {
            for (int poison = 0; poison < 3; ++poison) {
                g_state = (uint64_t)(n * 131 + shape * 17 + poison);
                std::vector<double> lower((size_t)(n * (n - 1) / 2));
                for (double& v : lower) v = 0.05 + rnd();
                if (poison == 1) lower[lower.size() / 2] = NAN;
                if (poison == 2) { lower[0] = INFINITY; lower[lower.size() - 1] = NAN; }
                std::vector<int32_t> mx((size_t)(n - 2)), my((size_t)(n - 2));
                for (int64_t it = 0; it < n - 2; ++it) {
                    const int64_t live = n - it;
                    const int64_t x = shape == 0 ? 0 : (int64_t)(rnd() * (double)(live - 1));
                    const int64_t y = shape == 0 ? 1 : x + 1 + (int64_t)(rnd() * (double)(live - 1 - x));
                    mx[(size_t)it] = (int32_t)x; my[(size_t)it] = (int32_t)y;
                }
                const int rounds = argc > 1 ? std::atoi(argv[1]) : 30;
                const int64_t M = 2 * n - 2;
                std::vector<int32_t> kids((size_t)(2 * (n - 2))), move((size_t)M), bw((size_t)(2 * M)), bk((size_t)(2 * M));
                std::vector<double> len((size_t)M), len2((size_t)M), gain((size_t)M), bg((size_t)(2 * M)), L((size_t)rounds + 1);
                int32_t top = -1;
                int64_t st[6] = { 0, 0, 0, 0, 0, 0 };
                double L2 = 0, L3 = 0;
                int rc = spr_host(lower.data(), n, mx.data(), my.data(), rounds, kids.data(), &top, len.data(), L.data(), st);
                if (rc == 0) rc = eval_host(lower.data(), n, kids.data(), top, len2.data(), gain.data(), move.data(), &L2);
                if (rc == 0) rc = spr_eval_host(lower.data(), n, kids.data(), top, -1, -1, bg.data(), bw.data(), bk.data(), &L3);
                // the tree the search ends on evaluates to the lengths it returned, bit for bit (NaN patterns included)
                bool same = rc == 0;
                for (size_t v = 0; same && v < len.size(); ++v) same = len[v] == len2[v] || (len[v] != len[v] && len2[v] != len2[v]);
                for (int64_t r = 1; same && r <= st[0]; ++r) same = L[(size_t)r] < L[(size_t)r - 1];
                // the single-move hook agrees with the scan: the best of d is one of its targets, with that gain
                int64_t targets = 0;
                if (same && n <= 33) {
                    for (int64_t d = 0; d < 2 * M; ++d) {
                        bool hit = bk[(size_t)d] == 0;
                        for (int32_t w = 0; w < M; ++w) {
                            double g = 0;
                            int32_t k = 0;
                            const int r1 = spr_eval_host(lower.data(), n, kids.data(), top, d, w, &g, nullptr, &k, nullptr);
                            same = same && (r1 == 0 || r1 == -2);
                            targets += r1 == 0;
                            if (r1 == 0 && w == bw[(size_t)d]) hit = g == bg[(size_t)d] && k == bk[(size_t)d];
                            if (r1 == 0 && g == g && bk[(size_t)d] != 0) same = same && !(g > bg[(size_t)d]);
                        }
                        same = same && hit;
                    }
                }
                std::printf("n %lld shape %d poison %d: rc %d rounds %lld moves %lld fallbacks %lld candidates %lld long %lld max_k %lld targets %lld L %.17g -> %.17g %s\n",
                            (long long)n, shape, poison, rc, (long long)st[0], (long long)st[1], (long long)st[2], (long long)st[3], (long long)st[4],
                            (long long)st[5], (long long)targets, L[0], L[(size_t)st[0]], same ? "ok" : "INCONSISTENT");
                bad += !same;
                // bad inputs are refused without touching memory they should not
                my[0] = (int32_t)n;
                bad += spr_host(lower.data(), n, mx.data(), my.data(), rounds, kids.data(), &top, len.data(), L.data(), st) != -1;
                if (n > 3) {
                    kids[0] = kids[1];
                    bad += spr_eval_host(lower.data(), n, kids.data(), top, -1, -1, bg.data(), bw.data(), bk.data(), &L3) != -1;
                }
            }
        }
    }
    return bad ? 2 : 0;
}
