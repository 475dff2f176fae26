// Balanced minimum evolution (Desper & Gascuel 2002): the parts of the NNI search that are the same on the host and on the device.
// Plain C++ (no HIP call, no library state), so that a stand-alone program can include it: the tree and its bookkeeping, the
// selection of a round's moves, the search loop, the per-node arithmetic (marked for both sides when hipcc compiles it) and the
// host engine behind dpr_bme_nni_host.  The contract is in include/dipper_hip.h above dpr_bme_nni; bme.hip holds the kernels.
//
// One square table T over the M = 2n - 2 nodes, row stride ld: T[u][v] = S(u, v) where neither node is an ancestor of the
// other (both orientations are kept), T[u][v] = W(u, v) where v is a proper ancestor of u.  T[v][u] of such a pair is unused.
// The host engine indexes T by node id; the device engine by the node's place in rank order (View::pos), which makes the rows
// of one height neighbours.  Which element holds a value has no part in the arithmetic.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#if defined(__HIPCC__)
#define DPR_BME_HD __host__ __device__
#else
#define DPR_BME_HD
#endif

namespace dpr {
namespace bme {

// the tree as the arithmetic reads it: seven arrays of M entries (kid0 = kid1 = -1 for tips; par[top] = t0, par[t0] = top)
struct View {
    const int32_t *kid0, *kid1, *par, *sib, *height, *tin, *tout;
    int32_t t0, top;
    const int32_t* pos;      // row / column of every node in T; null: its id
    DPR_BME_HD int64_t at(int32_t v) const { return pos ? pos[v] : v; }
};

DPR_BME_HD inline double avg2(double a, double b) { return 0.5 * (a + b); }
DPR_BME_HD inline bool in_clade(const View& t, int32_t u, int32_t v) { return t.tin[u] <= t.tin[v] && t.tin[v] < t.tout[u]; }   // v == u or below it

// W(u, v) for every proper ancestor v != t0 of u, from `top` down to parent(u), into row u of T.  The step bound only keeps a
// damaged tree from looping (a valid walk takes fewer than M steps).
DPR_BME_HD inline void walk_w(double* T, int64_t ld, int64_t M, const View& t, int32_t u)
{
    if (u == t.t0 || u == t.top) return;
    double* row = T + t.at(u) * ld;
    int32_t v = t.top;
    double w = row[t.at(t.t0)];
    row[t.at(v)] = w;
    for (int64_t step = 0; step < M; ++step) {
        const int32_t a = t.kid0[v], b = t.kid1[v];
        if (a < 0) return;
        const bool in_a = in_clade(t, a, u);
        const int32_t nxt = in_a ? a : b, other = in_a ? b : a;
        if (nxt == u) return;
        w = avg2(row[t.at(other)], w);
        row[t.at(nxt)] = w;
        v = nxt;
    }
}

// length of the edge above v, and the candidate move of v (move 0: v is no candidate)
DPR_BME_HD inline void eval_node(const double* T, int64_t ld, const View& t, int32_t v, double* len, double* gain, int32_t* move)
{
    *gain = 0.0; *move = 0; *len = 0.0;
    if (v == t.t0) return;
    const int32_t p = t.par[v], A = t.kid0[v], B = t.kid1[v];
    auto E = [&](int32_t r, int32_t c) { return T[t.at(r) * ld + t.at(c)]; };
    if (v == t.top) {
        *len = 0.5 * ((E(A, t.t0) + E(B, t.t0)) - E(A, B));
        return;
    }
    const int32_t C = t.sib[v];
    const double wcp = E(C, p);
    if (A < 0) {
        *len = 0.5 * ((E(v, C) + E(v, p)) - wcp);
        return;
    }
    const double sac = E(A, C), wap = E(A, p), sbc = E(B, C), wbp = E(B, p), sab = E(A, B);
    *len = 0.25 * (((sac + wap) + sbc) + wbp) - 0.5 * (sab + wcp);
    const double s0 = sab + wcp, s1 = sac + wbp, s2 = wap + sbc;
    const double g1 = 0.25 * (s0 - s1), g2 = 0.25 * (s0 - s2);
    const int32_t m = g1 >= g2 ? 1 : 2;
    const double g = m == 1 ? g1 : g2;
    *gain = g;
    *move = g > 0 ? m : 0;
}

// ---- host only from here ------------------------------------------------------------------------------------------------------
struct Tree {
    int64_t n = 0, M = 0;
    int32_t t0 = 0, top = 0, max_height = 0;
    std::vector<int32_t> kid0, kid1, par;                 // the topology
    std::vector<int32_t> sib, height, tin, tout;          // derived from it (derive)
    std::vector<int32_t> rows;                            // internal nodes by (height, id)
    std::vector<int32_t> pos;                             // place of every node in rank order: a tip its id, rows[k] the place n + k
    std::vector<int64_t> level;                           // rows of height h: [level[h], level[h + 1]), 1 <= h <= max_height
    std::vector<int32_t> stack;                           // scratch of derive
    View view() const { return View{ kid0.data(), kid1.data(), par.data(), sib.data(), height.data(), tin.data(), tout.data(), t0, top, nullptr }; }
};

// the tree of a merge log (the realID bookkeeping of writeNewickFromMerges), hung from tip n - 1; false: not a merge log
inline bool from_merges(int64_t n, const int32_t* mx, const int32_t* my, Tree& t)
{
    const int64_t M = 2 * n - 2;
    t.n = n; t.M = M; t.t0 = (int32_t)(n - 1);
    std::vector<int32_t> nb((size_t)(3 * M), -1), deg((size_t)M, 0), real((size_t)n);
    auto link = [&](int32_t a, int32_t b) {
        if (deg[(size_t)a] >= 3 || deg[(size_t)b] >= 3) return false;
        nb[(size_t)(3 * a + deg[(size_t)a]++)] = b;
        nb[(size_t)(3 * b + deg[(size_t)b]++)] = a;
        return true;
    };
    for (int64_t i = 0; i < n; ++i) real[(size_t)i] = (int32_t)i;
    for (int64_t it = 0; it < n - 2; ++it) {
        const int32_t x = mx[it], y = my[it];
        if (x < 0 || y <= x || y >= n - it) return false;
        const int32_t node = (int32_t)(n + it);
        if (!link(node, real[(size_t)x]) || !link(node, real[(size_t)y])) return false;
        real[(size_t)x] = node;
        real[(size_t)y] = real[(size_t)(n - it - 1)];
    }
    if (!link(real[0], real[1])) return false;
    t.kid0.assign((size_t)M, -1); t.kid1.assign((size_t)M, -1); t.par.assign((size_t)M, -1);
    t.top = nb[(size_t)(3 * t.t0)];
    t.par[(size_t)t.t0] = t.top; t.par[(size_t)t.top] = t.t0;
    t.stack.assign(1, t.top);
    while (!t.stack.empty()) {
        const int32_t v = t.stack.back();
        t.stack.pop_back();
        if (v < n) continue;
        int32_t k[2] = { -1, -1 }, c = 0;
        for (int e = 0; e < 3; ++e) {                        // (the three neighbours of a node are distinct: one is its parent)
            const int32_t w = nb[(size_t)(3 * v + e)];
            if (w < 0) return false;
            if (w == t.par[(size_t)v]) continue;
            if (c == 2) return false;
            k[c++] = w;
        }
        if (c != 2) return false;
        t.kid0[(size_t)v] = std::min(k[0], k[1]); t.kid1[(size_t)v] = std::max(k[0], k[1]);
        t.par[(size_t)k[0]] = t.par[(size_t)k[1]] = v;
        t.stack.push_back(k[0]); t.stack.push_back(k[1]);
    }
    return true;
}

// the tree of a children table as dpr_bme_nni writes it (kids of node n + k, the node next to tip n - 1); false: not a binary tree
inline bool from_kids(int64_t n, const int32_t* kids, int32_t top, Tree& t)
{
    const int64_t M = 2 * n - 2;
    t.n = n; t.M = M; t.t0 = (int32_t)(n - 1); t.top = top;
    if (top < n || top >= M) return false;
    t.kid0.assign((size_t)M, -1); t.kid1.assign((size_t)M, -1); t.par.assign((size_t)M, -1);
    t.par[(size_t)t.t0] = top; t.par[(size_t)top] = t.t0;
    for (int64_t k = 0; k < n - 2; ++k) {
        const int32_t a = kids[2 * k], b = kids[2 * k + 1];
        if (a < 0 || b < 0 || a >= M || b >= M || a == b || t.par[(size_t)a] != -1 || t.par[(size_t)b] != -1) return false;
        t.kid0[(size_t)(n + k)] = std::min(a, b); t.kid1[(size_t)(n + k)] = std::max(a, b);
        t.par[(size_t)a] = t.par[(size_t)b] = (int32_t)(n + k);
    }
    int64_t seen = 0;                                        // every node but t0 hangs below top
    t.stack.assign(1, top);
    while (!t.stack.empty()) {
        const int32_t v = t.stack.back();
        t.stack.pop_back();
        if (++seen > M) return false;
        if (v >= n) { t.stack.push_back(t.kid0[(size_t)v]); t.stack.push_back(t.kid1[(size_t)v]); }
    }
    return seen == M - 1;
}

// sib, height, tin / tout (pre-order intervals: t0 takes [0, 1), the clade of top [1, M)), rows and levels from the topology
inline void derive(Tree& t)
{
    const size_t M = (size_t)t.M;
    t.sib.assign(M, -1); t.height.assign(M, 0); t.tin.assign(M, 0); t.tout.assign(M, 0);
    t.tin[(size_t)t.t0] = 0; t.tout[(size_t)t.t0] = 1;
    int32_t clock = 1;
    t.stack.assign(1, t.top);
    while (!t.stack.empty()) {
        const int32_t e = t.stack.back();
        if (e >= 0) {                                        // entering e
            t.tin[(size_t)e] = clock++;
            t.stack.back() = ~e;
            if (t.kid0[(size_t)e] >= 0) {
                const int32_t a = t.kid0[(size_t)e], b = t.kid1[(size_t)e];
                t.sib[(size_t)a] = b; t.sib[(size_t)b] = a;
                t.stack.push_back(b); t.stack.push_back(a);
            }
        } else {                                             // leaving ~e
            const int32_t v = ~e;
            t.stack.pop_back();
            t.tout[(size_t)v] = clock;
            if (t.kid0[(size_t)v] >= 0) t.height[(size_t)v] = 1 + std::max(t.height[(size_t)t.kid0[(size_t)v]], t.height[(size_t)t.kid1[(size_t)v]]);
        }
    }
    t.max_height = t.height[(size_t)t.top];
    t.level.assign((size_t)t.max_height + 2, 0);
    for (int64_t v = t.n; v < t.M; ++v) ++t.level[(size_t)t.height[(size_t)v] + 1];
    for (size_t h = 1; h < t.level.size(); ++h) t.level[h] += t.level[h - 1];
    t.rows.resize((size_t)(t.n - 2));
    std::vector<int64_t> run(t.level.begin(), t.level.end());      // (running copy of the offsets)
    for (int64_t v = t.n; v < t.M; ++v) t.rows[(size_t)run[(size_t)t.height[(size_t)v]]++] = (int32_t)v;
    t.pos.resize(M);
    for (int64_t v = 0; v < t.n; ++v) t.pos[(size_t)v] = (int32_t)v;
    for (int64_t k = 0; k < t.n - 2; ++k) t.pos[(size_t)t.rows[(size_t)k]] = (int32_t)(t.n + k);
}

// move 1 of v exchanges its child kid1 with its sibling, move 2 its child kid0
inline void apply_move(Tree& t, int32_t v, int32_t move)
{
    const int32_t p = t.par[(size_t)v], A = t.kid0[(size_t)v], B = t.kid1[(size_t)v];
    const int32_t C = t.kid0[(size_t)p] == v ? t.kid1[(size_t)p] : t.kid0[(size_t)p];
    const int32_t X = move == 1 ? B : A, keep = move == 1 ? A : B;
    t.kid0[(size_t)v] = std::min(keep, C); t.kid1[(size_t)v] = std::max(keep, C);
    t.kid0[(size_t)p] = std::min(v, X); t.kid1[(size_t)p] = std::max(v, X);
    t.par[(size_t)X] = p; t.par[(size_t)C] = v;
}

// what one evaluation of a tree gives: per node the length of the edge above it, the gain and the move (0: no candidate); L
struct Eval {
    std::vector<double> len, gain;
    std::vector<int32_t> move;
    double L = 0.0;
    void size(int64_t M) { len.resize((size_t)M); gain.resize((size_t)M); move.resize((size_t)M); }
    void sum(int64_t M, int32_t t0)
    {
        L = 0.0;
        for (int64_t v = 0; v < M; ++v)
            if (v != t0) L += len[(size_t)v];
    }
};

inline bool better(const Eval& e, int32_t f, int32_t v)
{
    return e.gain[(size_t)f] > e.gain[(size_t)v] || (e.gain[(size_t)f] == e.gain[(size_t)v] && f < v);
}
// the selected candidates (ascending) and the best one; returns the number of candidates
inline int64_t select_moves(const Tree& t, const Eval& e, std::vector<int32_t>& sel, int32_t* best)
{
    int64_t cands = 0;
    sel.clear();
    *best = -1;
    for (int64_t q = t.n; q < t.M; ++q) {
        const int32_t v = (int32_t)q;
        if (!e.move[(size_t)v]) continue;
        ++cands;
        if (*best < 0 || better(e, v, *best)) *best = v;
        const int32_t rivals[4] = { t.par[(size_t)v], t.kid0[(size_t)v], t.kid1[(size_t)v], t.sib[(size_t)v] };
        bool beaten = false;
        for (int32_t f : rivals) beaten = beaten || (f >= 0 && e.move[(size_t)f] && better(e, f, v));
        if (!beaten) sel.push_back(v);
    }
    return cands;
}

// The search.  engine(tree, eval) evaluates a derived tree (0, or an error code that ends the search).  L_rounds may be null.
template <class Engine>
inline int search(Tree& t, int max_rounds, Engine&& engine, Eval& cur, double* L_rounds, int64_t* stats4)
{
    Eval nxt;
    cur.size(t.M); nxt.size(t.M);
    std::vector<int32_t> sel, moves, k0, k1, pr;
    int32_t best = -1;
    derive(t);
    if (int rc = engine(t, cur)) return rc;
    if (L_rounds) L_rounds[0] = cur.L;
    stats4[0] = stats4[1] = stats4[2] = 0;
    stats4[3] = select_moves(t, cur, sel, &best);
    for (int rounds = 0; rounds < max_rounds;) {
        if (select_moves(t, cur, sel, &best) == 0) break;
        moves.resize(sel.size());
        for (size_t i = 0; i < sel.size(); ++i) moves[i] = cur.move[(size_t)sel[i]];
        const int32_t best_move = cur.move[(size_t)best];
        k0 = t.kid0; k1 = t.kid1; pr = t.par;
        for (size_t i = 0; i < sel.size(); ++i) apply_move(t, sel[i], moves[i]);
        derive(t);
        if (int rc = engine(t, nxt)) return rc;
        int64_t applied = (int64_t)sel.size();
        if (!(nxt.L < cur.L)) {
            ++stats4[2];
            t.kid0 = k0; t.kid1 = k1; t.par = pr;
            apply_move(t, best, best_move);
            derive(t);
            if (int rc = engine(t, nxt)) return rc;
            applied = 1;
            if (!(nxt.L < cur.L)) {
                t.kid0 = k0; t.kid1 = k1; t.par = pr;
                derive(t);
                break;
            }
        }
        std::swap(cur, nxt);
        stats4[1] += applied;
        stats4[0] = ++rounds;
        if (L_rounds) L_rounds[rounds] = cur.L;
    }
    return 0;
}

inline void write_outputs(const Tree& t, const Eval& e, int32_t* kids, int32_t* top, double* len)
{
    for (int64_t k = 0; k < t.n - 2; ++k) {
        kids[2 * k] = t.kid0[(size_t)(t.n + k)];
        kids[2 * k + 1] = t.kid1[(size_t)(t.n + k)];
    }
    *top = t.top;
    for (int64_t v = 0; v < t.M; ++v) len[v] = v == t.t0 ? 0.0 : e.len[(size_t)v];
}

// ---- the host engine: the whole table in host memory, rows in rank order -------------------------------------------------------
struct HostEngine {
    std::vector<double> T;
    int64_t ld = 0;
    // tip against tip, once per search: lower_rows holds the strict lower triangle row by row
    void fill(int64_t n, const double* lower_rows)
    {
        ld = 2 * n - 2;
        T.assign((size_t)(ld * ld), 0.0);
        for (int64_t i = 1; i < n; ++i)
            for (int64_t j = 0; j < i; ++j) T[(size_t)(i * ld + j)] = T[(size_t)(j * ld + i)] = lower_rows[i * (i - 1) / 2 + j];
    }
    int operator()(const Tree& t, Eval& e)
    {
        const View w = t.view();
        double* Tp = T.data();
        for (int32_t u : t.rows) {
            const int32_t a = t.kid0[(size_t)u], b = t.kid1[(size_t)u], hu = t.height[(size_t)u];
            for (int32_t v = 0; v < t.M; ++v) {
                const int32_t hv = t.height[(size_t)v];
                if (!(hv < hu || (hv == hu && v < u)) || in_clade(w, u, v)) continue;
                Tp[(int64_t)u * ld + v] = Tp[(int64_t)v * ld + u] = avg2(Tp[(int64_t)a * ld + v], Tp[(int64_t)b * ld + v]);
            }
        }
        for (int32_t u = 0; u < t.M; ++u) walk_w(Tp, ld, t.M, w, u);
        for (int32_t v = 0; v < t.M; ++v) eval_node(Tp, ld, w, v, &e.len[(size_t)v], &e.gain[(size_t)v], &e.move[(size_t)v]);
        e.sum(t.M, t.t0);
        return 0;
    }
};

// dpr_bme_nni_host without the library around it: 0, or -1 (bad argument / not a merge log)
inline int nni_host(const double* lower_rows, int64_t n, const int32_t* mx, const int32_t* my, int max_rounds, int32_t* kids, int32_t* top,
                    double* len, double* L_rounds, int64_t* stats4)
{
    if (!lower_rows || n < 3 || n >= ((int64_t)1 << 30) || !mx || !my || max_rounds < 0 || !kids || !top || !len || !stats4) return -1;
    Tree t;
    if (!from_merges(n, mx, my, t)) return -1;
    HostEngine eng;
    eng.fill(n, lower_rows);
    Eval cur;
    if (int rc = search(t, max_rounds, eng, cur, L_rounds, stats4)) return rc;
    write_outputs(t, cur, kids, top, len);
    return 0;
}

// one evaluation of a given tree on the host (test hook dpr_bme_eval_host): 0, or -1
inline int eval_host(const double* lower_rows, int64_t n, const int32_t* kids, int32_t top, double* len, double* gain, int32_t* move, double* L)
{
    if (!lower_rows || n < 3 || n >= ((int64_t)1 << 30) || !kids || !len || !gain || !move || !L) return -1;
    Tree t;
    if (!from_kids(n, kids, top, t)) return -1;
    derive(t);
    HostEngine eng;
    eng.fill(n, lower_rows);
    Eval e;
    e.size(t.M);
    eng(t, e);
    std::copy(e.len.begin(), e.len.end(), len);
    std::copy(e.gain.begin(), e.gain.end(), gain);
    std::copy(e.move.begin(), e.move.end(), move);
    *L = e.L;
    return 0;
}

}  // namespace bme
}  // namespace dpr
