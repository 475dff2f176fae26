// Stand-alone driver of the tree fit's host side (fit_host.hpp), for builds with host sanitizers (`make fit_asan`): the restatement
// on caterpillars, balanced trees, a multifurcation and random merge logs through the three converters, with noisy, non-finite and
// zero entries; malformed trees and bad arguments.  No GPU, no library.  Prints one line per case; exit status 0 unless a result is
// inconsistent.
#include "fit_host.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>

static uint64_t g_state = 1;
static double rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

struct Arrays { std::vector<int32_t> parent; std::vector<double> len; int64_t m = 0; };

// a random merge log over n slots (merge_log.hpp): `merges` entries
static void random_log(int64_t n, int64_t merges, std::vector<int32_t>& mx, std::vector<int32_t>& my)
{
    mx.assign((size_t)(merges > 0 ? merges : 1), 0); my.assign(mx.size(), 1);
    for (int64_t it = 0; it < merges; ++it) {
        const int64_t live = n - it;
        int64_t x = (int64_t)(rnd() * (double)live), y = (int64_t)(rnd() * (double)(live - 1));
        if (x >= live) x = live - 1;
        if (y >= live - 1) y = live - 2;
        if (y >= x) ++y;
        mx[(size_t)it] = (int32_t)(x < y ? x : y); my[(size_t)it] = (int32_t)(x < y ? y : x);
    }
}

static Arrays tree_of(int shape, int64_t n)
{
    Arrays a;
    a.parent.assign((size_t)(2 * n - 1), -7); a.len.assign((size_t)(2 * n - 1), 0.0);
    std::vector<int32_t> mx, my;
    std::vector<double> bx((size_t)n), by((size_t)n), h((size_t)n);
    for (double& v : bx) v = 0.01 + rnd();
    for (double& v : by) v = rnd() < 0.1 ? -0.01 : rnd() < 0.1 ? 0.0 : 0.01 + rnd();
    if (shape == 0) {            // NJ log
        random_log(n, n - 2, mx, my);
        if (fit::from_nj(n, mx.data(), my.data(), bx.data(), by.data(), 0.3, a.parent.data(), a.len.data(), &a.m)) a.m = -1;
    } else if (shape == 1) {     // UPGMA log with rising heights
        random_log(n, n - 1, mx, my);
        double at = 0.0;
        for (int64_t it = 0; it < n - 1; ++it) { at += 0.01 + rnd(); h[(size_t)it] = at; }
        if (fit::from_upgma(n, mx.data(), my.data(), h.data(), a.parent.data(), a.len.data(), &a.m)) a.m = -1;
    } else if (shape == 2) {     // kids: a caterpillar hung from tip n - 1
        std::vector<int32_t> kids((size_t)(2 * (n > 2 ? n - 2 : 1)));
        std::vector<double> len_in((size_t)(2 * n - 2));
        for (double& v : len_in) v = 0.01 + rnd();
        // internal node n + k holds tip k + 1 and the node below it (n + k - 1, or tip 0 for k = 0)
        for (int64_t k = 0; k < n - 2; ++k) { kids[(size_t)(2 * k)] = (int32_t)(k == 0 ? 0 : n + k - 1); kids[(size_t)(2 * k + 1)] = (int32_t)(k + 1); }
        const int32_t top = (int32_t)(n == 2 ? 0 : 2 * n - 3);
        if (fit::from_kids(n, kids.data(), top, len_in.data(), a.parent.data(), a.len.data(), &a.m)) a.m = -1;
    } else {                     // a star with one cherry: m = n + 2 (n >= 4), else the star m = n + 1
        a.m = n >= 4 ? n + 2 : n + 1;
        a.parent.assign((size_t)a.m, (int32_t)n); a.len.assign((size_t)a.m, 0.0);
        for (int64_t v = 0; v < a.m; ++v) a.len[(size_t)v] = v == 1 ? INFINITY : 0.01 + rnd();
        a.parent[(size_t)n] = -1;
        if (n >= 4) { a.parent[0] = a.parent[2] = (int32_t)(n + 1); }
    }
    return a;
}

int main()
{
    const int64_t sizes[] = { 2, 3, 4, 5, 17, 64, 65, 257, 300 };
    int bad = 0;
    for (int64_t n : sizes)
        for (int shape = 0; shape < 4; ++shape) {
            g_state = (uint64_t)(n * 977 + shape);
            const Arrays a = tree_of(shape, n);
            if (a.m < 0) { std::printf("n %lld shape %d: converter refused its input INCONSISTENT\n", (long long)n, shape); ++bad; continue; }
            std::vector<double> lower((size_t)(n * (n - 1) / 2));
            for (double& v : lower) v = 0.05 + rnd();
            if (n >= 4) { lower[1] = NAN; lower[2] = INFINITY; lower[3] = 0.0; }
            std::vector<double> ss((size_t)n, -1.0);
            std::vector<int64_t> pairs((size_t)n, -1);
            double sums[fit::kSums];
            int32_t worst[2] = { -9, -9 };
            const int rc = fit::fit_host(lower.data(), n, a.m, a.parent.data(), a.len.data(), sums, ss.data(), pairs.data(), worst);
            // every pair is counted or skipped; a pair is in two taxa; the sums of squares of the taxa count every pair twice
            bool ok = rc == 0 && sums[fit::kN] + sums[fit::kSkipped] == (double)(n * (n - 1) / 2) && sums[fit::kNw] <= sums[fit::kN];
            int64_t twice = 0;
            double ss2 = 0.0;
            for (int64_t t = 0; t < n; ++t) { twice += pairs[(size_t)t]; ss2 += ss[(size_t)t]; ok = ok && ss[(size_t)t] >= 0.0; }
            ok = ok && (double)twice == 2.0 * sums[fit::kN] && std::fabs(ss2 - 2.0 * sums[fit::kSS]) <= 1e-9 * (1.0 + ss2);
            ok = ok && (sums[fit::kN] == 0.0 ? worst[0] == -1 : (worst[0] > worst[1] && worst[1] >= 0 && worst[0] < n));
            std::printf("n %lld shape %d m %lld: rc %d N %.0f skipped %.0f SS %.17g rms %.17g %s\n", (long long)n, shape, (long long)a.m, rc, sums[fit::kN],
                        sums[fit::kSkipped], sums[fit::kSS], sums[fit::kRms], ok ? "ok" : "INCONSISTENT");
            bad += !ok;
            // with the table: the same checks pass, the table's answers are the climbed ones
            fit::Topo t;
            bad += fit::prepare(n, a.m, a.parent.data(), a.len.data(), t, true) != 0;
            // malformed trees and bad arguments are refused before any output is written
            std::vector<int32_t> p2 = a.parent;
            p2[(size_t)t.root] = (int32_t)n == t.root ? (int32_t)(a.m - 1) : (int32_t)n;      // no root (or a cycle through it)
            bad += fit::prepare(n, a.m, p2.data(), a.len.data(), t, false) != -1;
            p2 = a.parent; p2[0] = 1;                                                          // a tip with a child
            bad += fit::prepare(n, a.m, p2.data(), a.len.data(), t, false) != -1;
            p2 = a.parent; p2[0] = (int32_t)a.m;                                               // a parent out of range
            bad += fit::prepare(n, a.m, p2.data(), a.len.data(), t, false) != -1;
            bad += fit::prepare(n, 2 * n, a.parent.data(), a.len.data(), t, false) != -1;
            bad += fit::prepare(1, 1, a.parent.data(), a.len.data(), t, false) != -1;
            bad += fit::fit_host(nullptr, n, a.m, a.parent.data(), a.len.data(), sums, ss.data(), pairs.data(), worst) != -1;
            bad += fit::fit_host(lower.data(), n, a.m, a.parent.data(), a.len.data(), sums, nullptr, pairs.data(), worst) != -1;
        }
    if (bad) std::printf("%d inconsistent\n", bad);
    return bad ? 2 : 0;
}
