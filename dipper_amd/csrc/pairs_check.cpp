// Stand-alone driver of pairs_host.hpp, for builds with host sanitizers (`make pairs_asan`): the pairs within a threshold and their
// labels on random triangles with NaN, +inf and -inf entries, at thresholds that keep nothing, one pair, a tenth and everything,
// with an output capacity of 0, of one entry and of all; each answer checked against a second formulation (a flood fill over the kept
// pairs); the summary of the labels; refused arguments.  No GPU, no library.  Prints one line per case; exit status 0 unless a result
// is inconsistent.
#include "pairs_host.hpp"

#include <cfloat>
#include <cstdio>

static uint64_t g_state = 1;
static double rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

int main()
{
    const int64_t sizes[] = { 2, 3, 5, 64, 65, 257, 300 };
    int bad = 0;
    for (int64_t n : sizes) {
        g_state = (uint64_t)(n * 7919);
        const int64_t cells = n * (n - 1) / 2;
        std::vector<double> lower((size_t)cells);
        for (double& v : lower) v = 0.01 * (double)(int)(rnd() * 100.0);      // two places: exact ties with the thresholds below
        if (n >= 5) { lower[1] = NAN; lower[2] = INFINITY; lower[3] = -INFINITY; lower[(size_t)cells - 1] = NAN; }
        const double thresholds[] = { 0.0, 0.1, 0.5, DBL_MAX };
        for (double T : thresholds) {
            int64_t want = 0;
            for (double v : lower) want += v <= T;
            int64_t count = -1, count0 = -1, count1 = -1;
            std::vector<int32_t> pi((size_t)(want ? want : 1), -1), pj(pi.size(), -1), label((size_t)n, -1), one_i(1, -1), one_j(1, -1);
            std::vector<double> pd(pi.size(), -1.0), one_d(1, -1.0);
            int rc = pairs::within_host(lower.data(), n, T, pi.data(), pj.data(), pd.data(), want, &count, label.data());
            rc |= pairs::within_host(lower.data(), n, T, nullptr, nullptr, nullptr, 0, &count0, nullptr);
            rc |= pairs::within_host(lower.data(), n, T, one_i.data(), one_j.data(), one_d.data(), 1, &count1, nullptr);
            bool ok = rc == 0 && count == want && count0 == want && count1 == want;
            // ordered, in range, the entry itself; the first pair alone where one entry was asked for
            for (int64_t k = 0; ok && k < want; ++k) {
                const int64_t a = pi[(size_t)k], b = pj[(size_t)k];
                ok = a > b && b >= 0 && a < n && pd[(size_t)k] == lower[(size_t)(a * (a - 1) / 2 + b)] && pd[(size_t)k] <= T;
                if (ok && k) ok = pi[(size_t)k - 1] < a || (pi[(size_t)k - 1] == a && pj[(size_t)k - 1] < b);
            }
            if (ok && want) ok = one_i[0] == pi[0] && one_j[0] == pj[0] && one_d[0] == pd[0];
            // the labels against a flood fill over the kept pairs, from every tip in ascending order
            std::vector<int32_t> fill((size_t)n, -1);
            for (int64_t s = 0; s < n; ++s) {
                if (fill[(size_t)s] >= 0) continue;
                std::vector<int64_t> todo(1, s);
                fill[(size_t)s] = (int32_t)s;
                while (!todo.empty()) {
                    const int64_t v = todo.back();
                    todo.pop_back();
                    for (int64_t k = 0; k < want; ++k) {
                        const int64_t w = pi[(size_t)k] == v ? pj[(size_t)k] : pj[(size_t)k] == v ? pi[(size_t)k] : -1;
                        if (w >= 0 && fill[(size_t)w] < 0) { fill[(size_t)w] = (int32_t)s; todo.push_back(w); }
                    }
                }
            }
            ok = ok && fill == label;
            int64_t sum[3] = { -1, -1, -1 };
            std::vector<int32_t> rank((size_t)n, -1);
            ok = ok && pairs::summarize(label.data(), n, sum, rank.data()) == 0 && sum[0] >= 1 && sum[0] <= n && sum[1] >= 1 && sum[2] <= sum[0];
            for (int64_t v = 0; ok && v < n; ++v) ok = rank[(size_t)v] >= 1 && rank[(size_t)v] <= sum[0] && rank[(size_t)v] == rank[(size_t)label[(size_t)v]];
            ok = ok && rank[0] == 1 && (want > 0 || (sum[0] == n && sum[2] == n && sum[1] == 1));
            std::printf("n %lld T %g: pairs %lld components %lld largest %lld singletons %lld %s\n", (long long)n, T, (long long)count, (long long)sum[0],
                        (long long)sum[1], (long long)sum[2], ok ? "ok" : "INCONSISTENT");
            bad += !ok;
        }
        // refused: nothing is written
        int64_t count = -5;
        std::vector<int32_t> label((size_t)n, -5);
        bad += pairs::within_host(nullptr, n, 0.1, nullptr, nullptr, nullptr, 0, &count, nullptr) != -1;
        bad += pairs::within_host(lower.data(), 1, 0.1, nullptr, nullptr, nullptr, 0, &count, nullptr) != -1;
        bad += pairs::within_host(lower.data(), n, NAN, nullptr, nullptr, nullptr, 0, &count, label.data()) != -1;
        bad += pairs::within_host(lower.data(), n, INFINITY, nullptr, nullptr, nullptr, 0, &count, label.data()) != -1;
        bad += pairs::within_host(lower.data(), n, -0.5, nullptr, nullptr, nullptr, 0, &count, label.data()) != -1;
        bad += pairs::within_host(lower.data(), n, 0.1, nullptr, nullptr, nullptr, 3, &count, label.data()) != -1;
        bad += pairs::within_host(lower.data(), n, 0.1, nullptr, nullptr, nullptr, 0, nullptr, label.data()) != -1;
        bad += count != -5 || label[0] != -5;
        int64_t sum[3];
        label.assign((size_t)n, 0);
        label[(size_t)n - 1] = (int32_t)(n - 1);
        label[0] = (int32_t)(n - 1);      // a label above its tip
        bad += pairs::summarize(label.data(), n, sum, nullptr) != -1;
    }
    if (bad) std::printf("%d inconsistent\n", bad);
    return bad ? 2 : 0;
}
