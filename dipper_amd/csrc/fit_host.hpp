// Fit of a tree to a distance matrix (residuals of the matrix against the tree's path lengths).  Contract: include/dipper_hip.h above
// dpr_tree_fit.  What the host restatement and the device pass share -- the tree as arrays and its checks, the depths, the terms of a
// pair, the combination of the per-row and per-column parts, the derived figures -- and the restatement itself (dpr_tree_fit_host),
// and the three converters from the builders' outputs: plain C++, no HIP, so that fit_check.cpp can build it under host sanitizers.
// The restatement finds lca(i, j) by CLIMBING the parent array from both tips; the device looks it up in a sparse table over the
// depth-first order of the tips (fit.hip), so that their agreement bit for bit means something.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "merge_log.hpp"

#if defined(__HIPCC__)
#define FIT_HD __host__ __device__
#else
#define FIT_HD
#endif

namespace fit {

constexpr int kRowAcc = 256;      // accumulators of a row part: term j goes to j mod 256
constexpr int kColAcc = 16;       // accumulators of a column part: term i goes to i mod 16
constexpr int kSums = 16;         // entries of `sums`
enum { kN = 0, kSkipped, kSumD, kSumP, kSumDD, kSumPP, kSumDP, kSS, kWSS, kNw, kMaxE, kRms, kRmsRel, kExplained, kCophenetic, kSpare };
constexpr int kRowSums = 7;       // sums kept per row: D, P, D D, P P, D P, e e, e e / (D D)

FIT_HD inline bool finite_d(double v) { return v - v == 0.0; }      // neither NaN nor an infinity
FIT_HD inline double patristic(double di, double dj, double da) { return (di - da) + (dj - da); }

// the terms of one pair; counted = false: nothing of it is added anywhere
struct Term {
    bool counted, weighted;
    double D, P, DD, PP, DP, ee, w, abs_e;
};
FIT_HD inline Term term_of(double D, double P)
{
    Term t;
    t.counted = finite_d(D) && finite_d(P);
    t.weighted = t.counted && D > 0.0;
    t.D = D; t.P = P;
    const double e = D - P;
    t.DD = D * D; t.PP = P * P; t.DP = D * P;
    t.ee = e * e;
    t.w = t.weighted ? t.ee / t.DD : 0.0;
    t.abs_e = e < 0.0 ? -e : e;
    return t;
}

// ---- the tree as arrays ----------------------------------------------------------------------------------------------------------
struct Topo {
    int64_t n = 0, m = 0;
    int32_t root = -1, height = 0;       // height: the most edges between the root and a node
    std::vector<int32_t> level;          // [m] edges between the root and the node
    std::vector<double> depth;           // [m] depth[root] = 0, depth[v] = depth[parent[v]] + len[v]
    std::vector<int32_t> rank;           // [n] place of every tip in the depth-first order (children ascending by node number)
    std::vector<int32_t> gap;            // [n - 1] order index of lca(tip of rank r, tip of rank r + 1)
    std::vector<double> dnode;           // [m - n] depth of the internal nodes by order index (ascending by level, then by number)
    int levels = 0;                      // rows of tab
    std::vector<int32_t> tab;            // [levels][n - 1]: tab[k][r] = min gap[r .. r + 2^k), where that range lies inside gap
};

// Checks (one root, which is internal; every other parent an internal node n <= p < m; every internal node with two children or more;
// every node reached from the root) and fills t.  0, or -1 for a malformed tree / a bad argument.
inline int prepare(int64_t n, int64_t m, const int32_t* parent, const double* len, Topo& t, bool with_table)
{
    if (!parent || !len || n < 2 || n >= ((int64_t)1 << 24) || m < n + 1 || m > 2 * n - 1) return -1;
    const size_t N = (size_t)n, M = (size_t)m, I = M - N;
    t.n = n; t.m = m; t.root = -1;
    std::vector<int32_t> first(I + 1, 0);      // children of internal node n + k: kid[first[k] .. first[k + 1])
    for (size_t v = 0; v < M; ++v) {
        const int64_t p = parent[v];
        if (p == -1) {
            if (t.root >= 0 || v < N) return -1;
            t.root = (int32_t)v;
            continue;
        }
        if (p < n || p >= m || p == (int64_t)v) return -1;
        ++first[(size_t)(p - n) + 1];
    }
    if (t.root < 0) return -1;
    for (size_t k = 0; k < I; ++k) {
        if (first[k + 1] < 2) return -1;
        first[k + 1] += first[k];
    }
    std::vector<int32_t> kid(M - 1), fill(first.begin(), first.end() - 1);
    for (size_t v = 0; v < M; ++v)
        if ((int32_t)v != t.root) kid[(size_t)fill[(size_t)(parent[v] - n)]++] = (int32_t)v;
    t.level.assign(M, -1);
    t.depth.assign(M, 0.0);
    t.rank.assign(N, -1);
    t.gap.assign(N - 1, -1);
    struct Frame { int32_t node, next; };
    std::vector<Frame> st;
    st.push_back(Frame{ t.root, 0 });
    t.level[(size_t)t.root] = 0;
    t.height = 0;
    size_t seen = 1, tips = 0;
    while (!st.empty()) {
        Frame& f = st.back();
        const size_t k = (size_t)(f.node - n);
        if (first[k] + f.next == first[k + 1]) { st.pop_back(); continue; }
        const int32_t c = kid[(size_t)(first[k] + f.next)];
        // between two consecutive tips of the order exactly one descent is not to a first child: from their lowest common ancestor
        if (f.next > 0) t.gap[tips - 1] = f.node;
        ++f.next;
        const int32_t lv = t.level[(size_t)f.node] + 1;
        t.level[(size_t)c] = lv;
        t.depth[(size_t)c] = t.depth[(size_t)f.node] + len[(size_t)c];
        if (lv > t.height) t.height = lv;
        ++seen;
        if ((size_t)c < N) t.rank[(size_t)c] = (int32_t)tips++;
        else st.push_back(Frame{ c, 0 });      // (f is not used after this)
    }
    if (seen != M || tips != N) return -1;      // a cycle hangs from no root: its nodes are never reached
    if (!with_table) return 0;
    // internal nodes ascending by level: the smallest order index of a range of gaps is its shallowest node, the range's lca
    std::vector<int32_t> at((size_t)t.height + 2, 0), order(I, 0);
    for (size_t k = 0; k < I; ++k) ++at[(size_t)t.level[N + k] + 1];
    for (size_t l = 0; l + 1 < at.size(); ++l) at[l + 1] += at[l];
    t.dnode.assign(I, 0.0);
    for (size_t k = 0; k < I; ++k) {
        order[k] = at[(size_t)t.level[N + k]]++;
        t.dnode[(size_t)order[k]] = t.depth[N + k];
    }
    for (size_t r = 0; r + 1 < N; ++r) t.gap[r] = order[(size_t)(t.gap[r] - n)];
    const size_t G = N - 1;
    t.levels = 1;
    while (((size_t)2 << (t.levels - 1)) <= G) ++t.levels;
    t.tab.assign((size_t)t.levels * G, 0);
    for (size_t r = 0; r < G; ++r) t.tab[r] = t.gap[r];
    for (int k = 1; k < t.levels; ++k) {
        const size_t half = (size_t)1 << (k - 1), span = half << 1;
        const int32_t* lo = &t.tab[(size_t)(k - 1) * G];
        int32_t* up = &t.tab[(size_t)k * G];
        for (size_t r = 0; r + span <= G; ++r) up[r] = lo[r] < lo[r + half] ? lo[r] : lo[r + half];
    }
    return 0;
}

// ---- parts and their combination -------------------------------------------------------------------------------------------------
// What the row pass and the column pass leave per taxon; combined by finish() on the host in both implementations.
struct Parts {
    std::vector<double> row;             // [kRowSums][n] row parts (pairs {i, j}, j < i)
    std::vector<int32_t> cnt;            // [3][n] of row i: counted pairs, counted pairs with D > 0, skipped pairs
    std::vector<double> max_e;           // [n] largest |e| of row i, -1 without a counted pair
    std::vector<int32_t> arg_j;          // [n] its smallest j
    std::vector<double> col_ss;          // [n] column part of e e (pairs {i, j}, i > j)
    std::vector<int32_t> col_cnt;        // [n] counted pairs of the column
    void size(size_t n)
    {
        row.assign(kRowSums * n, 0.0); cnt.assign(3 * n, 0); max_e.assign(n, -1.0); arg_j.assign(n, -1);
        col_ss.assign(n, 0.0); col_cnt.assign(n, 0);
    }
};

// the figures that follow from the sums; a zero denominator gives NaN (0 / 0)
inline void derive(double* s)
{
    const double N = s[kN], Nw = s[kNw], zero = 0.0;
    s[kRms] = N > 0.0 ? sqrt(s[kSS] / N) : zero / zero;
    s[kRmsRel] = Nw > 0.0 ? sqrt(s[kWSS] / Nw) : zero / zero;
    const double vd = N > 0.0 ? s[kSumDD] - s[kSumD] * s[kSumD] / N : 0.0;
    s[kExplained] = vd != 0.0 ? 1.0 - s[kSS] / vd : zero / zero;
    const double cd = N * s[kSumDD] - s[kSumD] * s[kSumD], cp = N * s[kSumPP] - s[kSumP] * s[kSumP];
    const double den = sqrt(cd * cp);
    s[kCophenetic] = den != 0.0 && den == den ? (N * s[kSumDP] - s[kSumD] * s[kSumP]) / den : zero / zero;
    s[kSpare] = 0.0;
}

// totals = the row parts added over i ascending; taxon_ss = row part + column part
inline void finish(int64_t n, const Parts& p, double* sums, double* taxon_ss, int64_t* taxon_pairs, int32_t* worst)
{
    const size_t N = (size_t)n;
    double tot[kRowSums] = { 0, 0, 0, 0, 0, 0, 0 };
    int64_t cnt = 0, cntw = 0, skipped = 0;
    double best = -1.0;
    worst[0] = worst[1] = -1;
    for (size_t i = 0; i < N; ++i) {
        for (int q = 0; q < kRowSums; ++q) tot[q] = tot[q] + p.row[(size_t)q * N + i];
        cnt += p.cnt[i]; cntw += p.cnt[N + i]; skipped += p.cnt[2 * N + i];
        if (p.max_e[i] > best) { best = p.max_e[i]; worst[0] = (int32_t)i; worst[1] = p.arg_j[i]; }
        taxon_ss[i] = p.row[(size_t)5 * N + i] + p.col_ss[i];
        taxon_pairs[i] = (int64_t)p.cnt[i] + (int64_t)p.col_cnt[i];
    }
    sums[kN] = (double)cnt; sums[kSkipped] = (double)skipped;
    sums[kSumD] = tot[0]; sums[kSumP] = tot[1]; sums[kSumDD] = tot[2]; sums[kSumPP] = tot[3]; sums[kSumDP] = tot[4];
    sums[kSS] = tot[5]; sums[kWSS] = tot[6];
    sums[kNw] = (double)cntw;
    sums[kMaxE] = best < 0.0 ? 0.0 : best;
    derive(sums);
}

template <int kAcc>
inline double halving_tree(double* a)
{
    for (int s = kAcc / 2; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t) a[t] = a[t] + a[t + s];
    return a[0];
}

// ---- the restatement ------------------------------------------------------------------------------------------------------------
// lower_rows: the strict lower triangle, row after row.  0, or -1 for a bad argument / a malformed tree.
inline int fit_host(const double* lower_rows, int64_t n, int64_t m, const int32_t* parent, const double* len, double* sums, double* taxon_ss,
                    int64_t* taxon_pairs, int32_t* worst)
{
    if (!lower_rows || !sums || !taxon_ss || !taxon_pairs || !worst) return -1;
    Topo t;
    if (prepare(n, m, parent, len, t, false)) return -1;
    const size_t N = (size_t)n;
    auto P_of = [&](size_t i, size_t j) {
        int32_t a = (int32_t)i, b = (int32_t)j;
        while (t.level[(size_t)a] > t.level[(size_t)b]) a = parent[a];
        while (t.level[(size_t)b] > t.level[(size_t)a]) b = parent[b];
        while (a != b) { a = parent[a]; b = parent[b]; }
        return patristic(t.depth[i], t.depth[j], t.depth[(size_t)a]);
    };
    Parts p;
    p.size(N);
    std::vector<double> acc((size_t)kRowSums * kRowAcc);
    for (size_t i = 0; i < N; ++i) {
        acc.assign(acc.size(), 0.0);
        const double* row = lower_rows + i * (i - 1) / 2;      // (i = 0: no entry is read)
        for (size_t j = 0; j < i; ++j) {
            const Term x = term_of(row[j], P_of(i, j));
            if (!x.counted) { ++p.cnt[2 * N + i]; continue; }
            const size_t c = j % kRowAcc;
            const double v[kRowSums] = { x.D, x.P, x.DD, x.PP, x.DP, x.ee, x.w };
            for (int q = 0; q < kRowSums; ++q)
                if (q != 6 || x.weighted) acc[(size_t)q * kRowAcc + c] = acc[(size_t)q * kRowAcc + c] + v[q];
            ++p.cnt[i];
            if (x.weighted) ++p.cnt[N + i];
            if (x.abs_e > p.max_e[i]) { p.max_e[i] = x.abs_e; p.arg_j[i] = (int32_t)j; }
        }
        for (int q = 0; q < kRowSums; ++q) p.row[(size_t)q * N + i] = halving_tree<kRowAcc>(&acc[(size_t)q * kRowAcc]);
    }
    for (size_t j = 0; j < N; ++j) {
        double a[kColAcc];
        for (int c = 0; c < kColAcc; ++c) a[c] = 0.0;
        for (size_t i = j + 1; i < N; ++i) {
            const Term x = term_of(lower_rows[i * (i - 1) / 2 + j], P_of(i, j));
            if (!x.counted) continue;
            a[i % kColAcc] = a[i % kColAcc] + x.ee;
            ++p.col_cnt[j];
        }
        p.col_ss[j] = halving_tree<kColAcc>(a);
    }
    finish(n, p, sums, taxon_ss, taxon_pairs, worst);
    return 0;
}

// ---- converters: the node bookkeeping of the command's Newick writers (merge_log.hpp) ------------------------------------------------
// All three give m = 2n - 1 nodes with the root last.  0, or -1 for a bad argument / an input that is no log or tree of its kind.

// NJ / BIONJ log (n - 2 merges, the lenient rule): merge_log::nj_edges, every edge written as parent[child], len[child]
inline int from_nj(int64_t n, const int32_t* mx, const int32_t* my, const double* bx, const double* by, double last, int32_t* parent, double* len,
                   int64_t* m)
{
    if (n < 2 || n >= ((int64_t)1 << 24) || !parent || !len || !m || (n > 2 && (!mx || !my || !bx || !by))) return -1;
    if (!merge_log::nj_edges<false>(n, mx, my, bx, by, last, [&](int32_t p, int, int32_t c, double l) { parent[c] = p; len[c] = l; })) return -1;
    const int64_t root = 2 * n - 2;
    parent[root] = -1; len[root] = 0.0;
    *m = 2 * n - 1;
    return 0;
}

// BME outputs (dpr_bme_nni / dpr_bme_spr): internal node n + k has the children kids[2k], kids[2k + 1]; len_in[v] is the edge above
// v < 2n - 2; tip n - 1 and `top` hang from the root 2n - 2, each on half of len_in[top]
inline int from_kids(int64_t n, const int32_t* kids, int32_t top, const double* len_in, int32_t* parent, double* len, int64_t* m)
{
    if (n < 2 || n >= ((int64_t)1 << 24) || !len_in || !parent || !len || !m || (n > 2 && !kids)) return -1;
    const int64_t M = 2 * n - 1, root = M - 1;
    if (top < 0 || top >= root || top == n - 1) return -1;
    for (int64_t v = 0; v < M; ++v) parent[v] = -2;
    for (int64_t k = 0; k < n - 2; ++k)
        for (int s = 0; s < 2; ++s) {
            const int64_t c = kids[2 * k + s];
            if (c < 0 || c >= root || c == n - 1 || c == top || parent[c] != -2) return -1;
            parent[c] = (int32_t)(n + k); len[c] = len_in[c];
        }
    if (parent[n - 1] != -2 || parent[top] != -2) return -1;
    parent[n - 1] = (int32_t)root; len[n - 1] = len_in[top] * 0.5;
    parent[top] = (int32_t)root; len[top] = len_in[top] * 0.5;
    parent[root] = -1; len[root] = 0.0;
    for (int64_t v = 0; v < M; ++v) if (parent[v] == -2) return -1;
    *m = M;
    return 0;
}

// UPGMA / WPGMA log (n - 1 merges with heights, the lenient rule): merge_log::upgma_edges, the last merge the root
inline int from_upgma(int64_t n, const int32_t* mx, const int32_t* my, const double* height, int32_t* parent, double* len, int64_t* m)
{
    if (n < 2 || n >= ((int64_t)1 << 24) || !mx || !my || !height || !parent || !len || !m) return -1;
    if (!merge_log::upgma_edges<false>(n, mx, my, height, [&](int32_t p, int, int32_t c, double l) { parent[c] = p; len[c] = l; })) return -1;
    const int64_t root = 2 * n - 2;
    parent[root] = -1; len[root] = 0.0;
    *m = 2 * n - 1;
    return 0;
}

}  // namespace fit
