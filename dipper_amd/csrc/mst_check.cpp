// Stand-alone driver of mst_host.hpp, for builds with host sanitizers (`make mst_asan`): the Kruskal forest of random triangles with
// ties, NaN, +inf, -inf, -0.0 and negative entries, unreachable groups and an isolated tip, checked against a second formulation (Prim
// from the first tip of every component: the smallest candidate under the same order with exactly one end in the tree, by a plain scan
// of the triangle); the dendrogram's log replayed by hand; refused arguments.  No GPU, no library.  Prints three lines per size; exit
// status 0 unless a result is inconsistent.
#include "mst_host.hpp"

#include <cstdio>

static uint64_t g_state = 1;
static double rnd()
{
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(g_state >> 11) / 9007199254740992.0;
}

int main()
{
    const int64_t sizes[] = { 2, 3, 5, 17, 64, 65, 130, 300 };
    int bad = 0;
    for (int64_t n : sizes) {
        g_state = (uint64_t)(n * 7919);
        const int64_t cells = n * (n - 1) / 2;
        std::vector<double> lower((size_t)cells);
        for (double& v : lower) v = 0.05 * (double)(int)(rnd() * 20.0) - 0.2;      // twenty values, four of them negative: ties everywhere
        auto cell = [&](int64_t a, int64_t b) -> double& { return lower[(size_t)(a * (a - 1) / 2 + b)]; };
        if (n >= 5) {
            cell(2, 1) = NAN; cell(3, 0) = INFINITY; cell(3, 1) = -INFINITY; cell(n - 1, n - 2) = NAN;
            cell(3, 2) = -0.0; cell(4, 0) = 0.0; cell(4, 1) = -0.0;
        }
        if (n >= 17) {
            for (int64_t a = 0; a < n; ++a)      // tip 7 reaches nobody; the tips from 3 n / 4 on reach nobody below
                for (int64_t b = 0; b < a; ++b)
                    if (a == 7 || b == 7 || (a >= 3 * n / 4 && b < 3 * n / 4)) cell(a, b) = (a + b) % 2 ? NAN : INFINITY;
        }
        std::vector<int32_t> ei((size_t)n, -7), ej((size_t)n, -7), label((size_t)n, -7);
        std::vector<double> ed((size_t)n, -7.0);
        int64_t E = -7;
        bool ok = mst::mst_host(lower.data(), n, ei.data(), ej.data(), ed.data(), &E, label.data()) == 0 && E >= 0 && E <= n - 1;
        // Prim per component
        std::vector<char> in((size_t)n, 0);
        std::vector<mst::Edge> prim;
        int64_t comps = 0;
        for (int64_t start = 0; ok && start < n; ++start) {
            if (in[(size_t)start]) continue;
            ++comps;
            in[(size_t)start] = 1;
            ok = label[(size_t)start] == (int32_t)start;
            for (;;) {
                mst::Edge best{ 0, -1, -1, 0.0 };
                for (int64_t a = 1; a < n; ++a)
                    for (int64_t b = 0; b < a; ++b) {
                        // (the earlier components are closed: no finite entry leaves them, so one end in the tree means THIS tree)
                        if (in[(size_t)a] == in[(size_t)b] || !std::isfinite(cell(a, b))) continue;
                        const mst::Edge e{ mst::key_of(cell(a, b)), (int32_t)a, (int32_t)b, cell(a, b) };
                        if (best.i < 0 || mst::before(e, best)) best = e;
                    }
                if (best.i < 0) break;
                in[(size_t)best.i] = in[(size_t)best.j] = 1;
                prim.push_back(best);
            }
        }
        // no finite entry leaves a component, and every tip of a component was reached
        for (int64_t a = 1; ok && a < n; ++a)
            for (int64_t b = 0; b < a; ++b)
                if (std::isfinite(cell(a, b)) && label[(size_t)a] != label[(size_t)b]) ok = false;
        for (int64_t v = 0; ok && v < n; ++v) ok = in[(size_t)v] && label[(size_t)v] <= (int32_t)v;
        std::sort(prim.begin(), prim.end(), mst::before);
        ok = ok && (int64_t)prim.size() == E && E == n - comps;
        for (int64_t t = 0; ok && t < E; ++t)
            ok = prim[(size_t)t].i == ei[(size_t)t] && prim[(size_t)t].j == ej[(size_t)t] && mst::bits_of(prim[(size_t)t].d) == mst::bits_of(ed[(size_t)t]) &&
                 ei[(size_t)t] > ej[(size_t)t];
        // the library's order-and-check of a shuffled copy gives the same forest back
        if (ok && E > 1) {
            std::vector<int32_t> si(ei.begin(), ei.begin() + E), sj(ej.begin(), ej.begin() + E), sl((size_t)n);
            std::vector<double> sd(ed.begin(), ed.begin() + E);
            for (int64_t t = E - 1; t > 0; --t) {
                const int64_t u = (int64_t)(rnd() * (double)(t + 1));
                std::swap(si[(size_t)t], si[(size_t)u]); std::swap(sj[(size_t)t], sj[(size_t)u]); std::swap(sd[(size_t)t], sd[(size_t)u]);
            }
            ok = mst::order_and_label(n, si.data(), sj.data(), sd.data(), E, sl.data()) == 0 && sl == label;
            for (int64_t t = 0; ok && t < E; ++t) ok = si[(size_t)t] == ei[(size_t)t] && sj[(size_t)t] == ej[(size_t)t];
            si[0] = si[1]; sj[0] = sj[1];      // an edge twice: no forest
            ok = ok && mst::order_and_label(n, si.data(), sj.data(), sd.data(), E, sl.data()) == -1;
        }
        std::printf("n %lld: %lld edges, %lld components %s\n", (long long)n, (long long)E, (long long)comps, ok ? "ok" : "INCONSISTENT");
        bad += !ok;

        // the dendrogram of a connected input (the same values, nothing non-finite): the log replayed over slots by hand
        for (double& v : lower)
            if (!std::isfinite(v)) v = 0.9;
        std::vector<int32_t> mx((size_t)n, -7), my((size_t)n, -7);
        std::vector<double> h((size_t)n, -7.0);
        ok = mst::mst_host(lower.data(), n, ei.data(), ej.data(), ed.data(), &E, label.data()) == 0 && E == n - 1;
        ok = ok && mst::dendrogram_host(n, ei.data(), ej.data(), ed.data(), E, mx.data(), my.data(), h.data()) == 0;
        std::vector<std::vector<int32_t>> members((size_t)n);      // tips of the node in every slot
        for (int64_t v = 0; v < n; ++v) members[(size_t)v] = { (int32_t)v };
        for (int64_t t = 0; ok && t < n - 1; ++t) {
            const int64_t x = mx[(size_t)t], y = my[(size_t)t], live = n - t;
            ok = x >= 0 && x < y && y < live && h[(size_t)t] == 0.5 * ed[(size_t)t];
            if (!ok) break;
            auto holds = [&](int64_t slot, int32_t tip) { return std::find(members[(size_t)slot].begin(), members[(size_t)slot].end(), tip) != members[(size_t)slot].end(); };
            ok = (holds(x, ei[(size_t)t]) && holds(y, ej[(size_t)t])) || (holds(x, ej[(size_t)t]) && holds(y, ei[(size_t)t]));
            members[(size_t)x].insert(members[(size_t)x].end(), members[(size_t)y].begin(), members[(size_t)y].end());
            members[(size_t)y] = members[(size_t)(live - 1)];
        }
        ok = ok && (int64_t)members[0].size() == n;
        std::printf("n %lld: dendrogram of %lld merges %s\n", (long long)n, (long long)(n - 1), ok ? "ok" : "INCONSISTENT");
        bad += !ok;

        // refused: nothing is written
        std::vector<int32_t> qi((size_t)n, -5), qj((size_t)n, -5), ql((size_t)n, -5);
        std::vector<double> qd((size_t)n, -5.0);
        int64_t qe = -5;
        int refused = 0;
        refused += mst::mst_host(nullptr, n, qi.data(), qj.data(), qd.data(), &qe, ql.data()) == -1;
        refused += mst::mst_host(lower.data(), 1, qi.data(), qj.data(), qd.data(), &qe, ql.data()) == -1;
        refused += mst::mst_host(lower.data(), n, nullptr, qj.data(), qd.data(), &qe, ql.data()) == -1;
        refused += mst::mst_host(lower.data(), n, qi.data(), nullptr, qd.data(), &qe, ql.data()) == -1;
        refused += mst::mst_host(lower.data(), n, qi.data(), qj.data(), nullptr, &qe, ql.data()) == -1;
        refused += mst::mst_host(lower.data(), n, qi.data(), qj.data(), qd.data(), nullptr, ql.data()) == -1;
        refused += mst::mst_host(lower.data(), n, qi.data(), qj.data(), qd.data(), &qe, nullptr) == -1;
        refused += mst::dendrogram_host(n, ei.data(), ej.data(), ed.data(), E - 1, qi.data(), qj.data(), qd.data()) == -1;
        refused += mst::dendrogram_host(1, ei.data(), ej.data(), ed.data(), 0, qi.data(), qj.data(), qd.data()) == -1;
        refused += mst::dendrogram_host(n, ei.data(), ej.data(), ed.data(), E, nullptr, qj.data(), qd.data()) == -1;
        ok = refused == 10 && qi[0] == -5 && qj[0] == -5 && qd[0] == -5.0 && ql[0] == -5 && qe == -5;
        std::printf("n %lld: refused arguments %s\n", (long long)n, ok ? "ok" : "INCONSISTENT");
        bad += !ok;
    }
    if (bad) std::printf("%d inconsistent\n", bad);
    return bad ? 2 : 0;
}
