// Balanced minimum evolution (Desper & Gascuel 2002): the parts of the NNI and SPR searches that are the same on the host and on the device.
// Plain C++ (no HIP call, no library state), so that a stand-alone program can include it: the tree and its bookkeeping, the
// selection of a round's moves, the search loop, the per-node arithmetic (marked for both sides when hipcc compiles it) and the
// host engine behind dpr_bme_nni_host.  The contract is in include/dipper_hip.h above dpr_bme_nni; bme.hip holds the kernels.
//
// One square table T over the M = 2n - 2 nodes, row stride ld: T[u][v] = S(u, v) where neither node is an ancestor of the
// other (both orientations are kept), T[u][v] = W(u, v) where v is a proper ancestor of u.  T[v][u] of such a pair is unused by
// the NNI search; the SPR scan mirrors W into it (spr_mirror_w below).
// The host engine indexes T by node id; the device engine by the node's place in rank order (View::pos), which makes the rows
// of one height neighbours.  Which element holds a value has no part in the arithmetic.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "merge_log.hpp"

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

// the tree of a merge log (merge_log.hpp, the strict rule), hung from tip n - 1; false: not a merge log
inline bool from_merges(int64_t n, const int32_t* mx, const int32_t* my, Tree& t)
{
    const int64_t M = 2 * n - 2;
    t.n = n; t.M = M; t.t0 = (int32_t)(n - 1);
    std::vector<int32_t> nb((size_t)(3 * M), -1), deg((size_t)M, 0), real;
    bool linked = true;
    auto link = [&](int32_t a, int32_t b) {
        if (deg[(size_t)a] >= 3 || deg[(size_t)b] >= 3) { linked = false; return; }
        nb[(size_t)(3 * a + deg[(size_t)a]++)] = b;
        nb[(size_t)(3 * b + deg[(size_t)b]++)] = a;
    };
    if (!merge_log::replay<true>(n, n - 2, mx, my, real, [&](int64_t, int32_t node, int32_t u, int32_t v) { link(node, u); link(node, v); }))
        return false;
    link(real[0], real[1]);
    if (!linked) return false;
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

// ---- SPR (subtree pruning and regrafting): the contract is in include/dipper_hip.h above dpr_bme_spr ----------------------------
// The scan reads T through the unordered pair of the two subtrees' nodes: the subtree seen from p towards a neighbour is named by
// the lower node of that edge (the clade of a child, or everything outside the clade of p; outside the clade of `top` is the tip
// t0).  Two disjoint subtrees' nodes are either unrelated (S) or one is an ancestor of the other (W), so once W is mirrored into
// the elements T[ancestor][node], which nothing else reads, T[a][b] is the average of the pair in either orientation.
DPR_BME_HD inline void spr_mirror_w(double* T, int64_t ld, int64_t M, const View& t, int32_t u)
{
    if (u == t.t0 || u == t.top) return;
    const int64_t cu = t.at(u);
    int32_t v = t.par[u];
    for (int64_t step = 0; step < M && v != t.t0; ++step) {
        const int64_t cv = t.at(v);
        T[cv * ld + cu] = T[cu * ld + cv];
        v = t.par[v];
    }
}

// one node as the scan reads it: children (-1: a tip), parent, nodes in its clade -- in the index space of T
struct SprRec { int32_t k0, k1, par, size; };
struct SprTree {
    const double* T;
    int64_t ld;
    const SprRec* rec;
    const int32_t* ids;      // node id of every index; null: itself
    const double* trio;      // per node p three averages between the subtrees at p: (k0, k1), (k0, outside p), (k1, outside p); null: read from T
    int32_t n, M, t0, top;   // tips are the indices below n in either space
    DPR_BME_HD int32_t id(int32_t v) const { return ids ? ids[v] : v; }
    DPR_BME_HD int32_t lower(int32_t c) const { return id(c == t0 ? top : c); }      // the edge at t0 is the one above `top`
};

// the best target of one pruned subtree so far (k = 0: none); want >= 0: the gain of that target alone, whatever it is
struct SprBest {
    double g = 0.0;
    int32_t w = -1, k = 0, want = -1;
    DPR_BME_HD void merge(double g2, int32_t w2, int32_t k2)      // w2: a node id
    {
        if (k == 0 || g2 > g || (g2 == g && w2 < w)) { g = g2; w = w2; k = k2; }
    }
    DPR_BME_HD void take(const SprTree& t, double g2, int32_t wplace, int32_t k2)
    {
        if (want >= 0) {
            if (t.lower(wplace) == want) { g = g2; w = want; k = k2; }
            return;
        }
        if (!(g2 == g2) || (k != 0 && !(g2 >= g))) return;
        merge(g2, t.lower(wplace), k2);
    }
};

// where one traversal stands: the rows of X and A, d(X, A), and the path node to visit next with the sums of the path before it
struct SprState {
    int64_t xr, ar;
    double dXA, U, V, h;
    int32_t p, from, k;
};

// the two neighbours of a node other than x, in the order (k0, k1, par)
DPR_BME_HD inline void spr_others(const SprRec& r, int32_t x, int32_t* o0, int32_t* o1)
{
    if (x == r.k0) { *o0 = r.k1; *o1 = r.par; }
    else if (x == r.k1) { *o0 = r.k0; *o1 = r.par; }
    else { *o0 = r.k0; *o1 = r.k1; }
}

DPR_BME_HD inline double spr_gain(double h, double dXA, double xB, double Uk, double Vk, double yB, double cB, double aB)
{
    return (((0.5 - h) * (dXA - xB) + (Uk - Vk)) + 0.25 * (yB + cB)) - (0.5 * h) * (aB + xB);
}

// Directed subtree dp (index v: the clade of v; M + v: outside the clade of v), direction 0 / 1 = which of q's two other
// neighbours the path leaves through.  false: not prunable, or nothing to visit that way.
DPR_BME_HD inline bool spr_begin(const SprTree& t, int32_t dp, int dir, SprState& s)
{
    const bool outside = dp >= t.M;
    const int32_t v = outside ? dp - t.M : dp;
    const SprRec rv = t.rec[v];
    int32_t x0, q, xnode;
    if (!outside) {
        if (v == t.t0 || v == t.top) return false;
        x0 = v; q = rv.par; xnode = v;
    } else {
        if (rv.k0 < 0) return false;
        q = v; x0 = rv.par; xnode = v == t.top ? t.t0 : v;
    }
    const SprRec rq = t.rec[q];
    int32_t o0, o1;
    spr_others(rq, x0, &o0, &o1);
    const int32_t p1 = dir ? o1 : o0, a0 = dir ? o0 : o1;
    if (p1 < t.n) return false;
    const int32_t anode = (a0 != rq.par || q == t.top) ? a0 : q;
    s.xr = (int64_t)xnode * t.ld; s.ar = (int64_t)anode * t.ld;
    s.dXA = t.T[s.xr + anode];
    s.U = 0.0; s.V = 0.0; s.h = 0.5;
    s.p = p1; s.from = q; s.k = 0;
    return true;
}

// Visit path node s.p: its two targets, then on to the next path node -- the smaller of two internal continuations first, the
// larger one stacked, which keeps the stack below log2 M entries.  false: the traversal is over.
template <class Stack>
DPR_BME_HD inline bool spr_step(const SprTree& t, SprState& s, SprBest& b, Stack& st)
{
    const int32_t p = s.p;
    const SprRec r = t.rec[p];
    int32_t n1, n2;
    spr_others(r, s.from, &n1, &n2);
    const bool attop = p == t.top;
    const int32_t c1 = (n1 != r.par || attop) ? n1 : p, c2 = (n2 != r.par || attop) ? n2 : p, cc = (s.from != r.par || attop) ? s.from : p;
    const int32_t k = s.k + 1;
    const double h = 0.5 * s.h;
    const double* T = t.T;
    const double x1 = T[s.xr + c1], x2 = T[s.xr + c2], a1 = T[s.ar + c1], a2 = T[s.ar + c2];
    double y, cb1, cb2;                                      // d(Y_k, B) and d(C_k, B) of the two targets: the same for every X
    if (t.trio) {
        const double* q3 = t.trio + 3 * (int64_t)p;
        const double d01 = q3[0], d0p = q3[1], d1p = q3[2];
        if (s.from == r.k0) { y = d1p; cb1 = d01; cb2 = d0p; }
        else if (s.from == r.k1) { y = d0p; cb1 = d01; cb2 = d1p; }
        else { y = d01; cb1 = d0p; cb2 = d1p; }
    } else {
        y = T[(int64_t)c1 * t.ld + c2]; cb1 = T[(int64_t)cc * t.ld + c1]; cb2 = T[(int64_t)cc * t.ld + c2];
    }
    const double U1 = s.U + h * (x2 - a2), V1 = 0.5 * s.V + 0.25 * x2;      // on towards n1: Y_k is beyond n2
    const double U2 = s.U + h * (x1 - a1), V2 = 0.5 * s.V + 0.25 * x1;      // on towards n2
    b.take(t, spr_gain(h, s.dXA, x1, U1, V1, y, cb1, a1), c1, k);
    b.take(t, spr_gain(h, s.dXA, x2, U2, V2, y, cb2, a2), c2, k);
    const bool i1 = n1 >= t.n, i2 = n2 >= t.n;
    if (i1 && i2) {
        const int32_t s1 = c1 == n1 ? t.rec[n1].size : t.M - r.size, s2 = c2 == n2 ? t.rec[n2].size : t.M - r.size;
        const bool first1 = s1 <= s2;
        st.push(first1 ? n2 : n1, p, k, first1 ? U2 : U1, first1 ? V2 : V1, h);
        s.p = first1 ? n1 : n2; s.U = first1 ? U1 : U2; s.V = first1 ? V1 : V2;
    } else if (i1 || i2) {
        s.p = i1 ? n1 : n2; s.U = i1 ? U1 : U2; s.V = i1 ? V1 : V2;
    } else {
        return st.pop(s);
    }
    s.from = p; s.k = k; s.h = h;
    return true;
}

// ---- host only from here ------------------------------------------------------------------------------------------------------
constexpr int kSprStack = 32;      // log2 M < 25 entries are ever held (n < 2^24)
struct SprHostStack {
    struct Entry { double U, V, h; int32_t p, from, k; } e[kSprStack];
    int sp = 0;
    void push(int32_t p, int32_t from, int32_t k, double U, double V, double h)
    {
        if (sp < kSprStack) e[sp++] = Entry{ U, V, h, p, from, k };
    }
    bool pop(SprState& s)
    {
        if (sp == 0) return false;
        const Entry& x = e[--sp];
        s.U = x.U; s.V = x.V; s.h = x.h; s.p = x.p; s.from = x.from; s.k = x.k;
        return true;
    }
};

// per directed subtree d (2M entries): gain, target w and path length k of its best target (k = 0: none, gain 0, w -1)
struct SprEval {
    std::vector<double> gain;
    std::vector<int32_t> w, k;
    void size(int64_t M) { gain.resize((size_t)(2 * M)); w.resize((size_t)(2 * M)); k.resize((size_t)(2 * M)); }
};

// the scan's view of a derived tree: 4 M ints of records at out, M ints of node ids at out + ids_off.  places: in rank-order
// places (the device table), else in node ids (the host table)
inline void spr_records(const Tree& t, bool places, int32_t* out, int64_t ids_off)
{
    for (int64_t v = 0; v < t.M; ++v) {
        auto at = [&](int32_t u) { return u < 0 || !places ? u : t.pos[(size_t)u]; };
        const int64_t p = at((int32_t)v);
        out[4 * p] = at(t.kid0[(size_t)v]); out[4 * p + 1] = at(t.kid1[(size_t)v]); out[4 * p + 2] = at(t.par[(size_t)v]);
        out[4 * p + 3] = t.tout[(size_t)v] - t.tin[(size_t)v];
        out[ids_off + p] = (int32_t)v;
    }
}

inline void spr_scan_one(const SprTree& st, int32_t d, SprBest& b)
{
    for (int dir = 0; dir < 2; ++dir) {
        SprState s;
        SprHostStack stack;
        bool live = spr_begin(st, d, dir, s);
        for (int64_t step = 0; live && step < st.M; ++step) live = spr_step(st, s, b, stack);
    }
}

// the nodes of the move (d, w): x0, a0, q, p_1 .. p_k, b0 appended to out; returns k
inline int32_t spr_path(const Tree& t, int32_t d, int32_t w, std::vector<int32_t>& out)
{
    const View vw = t.view();
    const bool outside = d >= t.M;
    const int32_t v = outside ? d - (int32_t)t.M : d;
    const int32_t x0 = outside ? t.par[(size_t)v] : v, q = outside ? v : t.par[(size_t)v];
    const size_t base = out.size();
    out.push_back(x0); out.push_back(-1); out.push_back(q);
    int32_t b0;
    if (in_clade(vw, w, q)) {                                // w is above q: up to w, the target is the edge above it
        for (int32_t a = q; a != w;) { a = t.par[(size_t)a]; out.push_back(a); }
        b0 = t.par[(size_t)w];
    } else {                                                 // up to the last common ancestor, then down to parent(w)
        int32_t a = q;
        while (!in_clade(vw, a, w)) { a = t.par[(size_t)a]; out.push_back(a); }
        const size_t mid = out.size();
        for (int32_t c = t.par[(size_t)w]; c != a; c = t.par[(size_t)c]) out.push_back(c);
        std::reverse(out.begin() + (std::ptrdiff_t)mid, out.end());
        b0 = w;
    }
    out.push_back(b0);
    const int32_t p1 = out[base + 3];
    const int32_t nbq[3] = { t.kid0[(size_t)q], t.kid1[(size_t)q], t.par[(size_t)q] };
    for (int32_t c : nbq)
        if (c != x0 && c != p1) out[base + 1] = c;
    return (int32_t)(out.size() - base) - 4;
}

// the moves of a round: node sets one after another in `nodes`, move i at [off[i], off[i + 1]), its subtree d[i]
struct SprMoves {
    std::vector<int32_t> nodes, d;
    std::vector<size_t> off;
    std::vector<int32_t> order;
    std::vector<uint8_t> mark;
    size_t count() const { return d.size(); }
    int32_t k(size_t i) const { return (int32_t)(off[i + 1] - off[i]) - 4; }
};

// candidates by (gain descending, d ascending), each selected iff its nodes are free; returns the number of candidates
inline int64_t spr_select(const Tree& t, const SprEval& e, SprMoves& m)
{
    m.nodes.clear(); m.d.clear(); m.off.assign(1, 0); m.order.clear();
    m.mark.assign((size_t)t.M, 0);
    for (int64_t d = 0; d < 2 * t.M; ++d)
        if (e.k[(size_t)d] != 0 && e.gain[(size_t)d] > 0) m.order.push_back((int32_t)d);
    std::sort(m.order.begin(), m.order.end(), [&](int32_t a, int32_t b) {
        return e.gain[(size_t)a] > e.gain[(size_t)b] || (e.gain[(size_t)a] == e.gain[(size_t)b] && a < b);
    });
    for (int32_t d : m.order) {
        const size_t base = m.nodes.size();
        spr_path(t, d, e.w[(size_t)d], m.nodes);
        bool is_free = true;
        for (size_t i = base; i < m.nodes.size(); ++i) is_free = is_free && !m.mark[(size_t)m.nodes[i]];
        if (!is_free) { m.nodes.resize(base); continue; }
        for (size_t i = base; i < m.nodes.size(); ++i) m.mark[(size_t)m.nodes[i]] = 1;
        m.d.push_back(d);
        m.off.push_back(m.nodes.size());
    }
    return (int64_t)m.order.size();
}

// moves [first, last) applied to the unrooted tree (q leaves between a0 and p_1 and enters between p_k and b0), re-hung from t0
inline bool spr_apply(Tree& t, const SprMoves& m, size_t first, size_t last, std::vector<int32_t>& nb)
{
    const int64_t M = t.M;
    nb.assign((size_t)(3 * M), -1);
    for (int64_t v = 0; v < M; ++v) {
        nb[(size_t)(3 * v)] = t.par[(size_t)v];
        nb[(size_t)(3 * v + 1)] = t.kid0[(size_t)v];
        nb[(size_t)(3 * v + 2)] = t.kid1[(size_t)v];
    }
    auto rep = [&](int32_t node, int32_t old, int32_t nw) {
        for (int e = 0; e < 3; ++e)
            if (nb[(size_t)(3 * node + e)] == old) { nb[(size_t)(3 * node + e)] = nw; return; }
    };
    for (size_t i = first; i < last; ++i) {
        const int32_t* s = m.nodes.data() + m.off[i];
        const size_t cnt = m.off[i + 1] - m.off[i];
        const int32_t a0 = s[1], q = s[2], p1 = s[3], pk = s[cnt - 2], b0 = s[cnt - 1];
        rep(a0, q, p1); rep(p1, q, a0);
        rep(pk, b0, q); rep(b0, pk, q);
        rep(q, a0, b0);
        if (p1 != pk) rep(q, p1, pk);
    }
    t.kid0.assign((size_t)M, -1); t.kid1.assign((size_t)M, -1); t.par.assign((size_t)M, -1);
    t.top = nb[(size_t)(3 * t.t0)];
    if (t.top < t.n) return false;
    t.par[(size_t)t.t0] = t.top; t.par[(size_t)t.top] = t.t0;
    t.stack.assign(1, t.top);
    int64_t seen = 0;
    while (!t.stack.empty()) {
        const int32_t v = t.stack.back();
        t.stack.pop_back();
        if (++seen > M) return false;
        if (v < t.n) continue;
        int32_t k[2] = { -1, -1 }, c = 0;
        for (int e = 0; e < 3; ++e) {
            const int32_t u = nb[(size_t)(3 * v + e)];
            if (u == t.par[(size_t)v]) continue;
            if (u < 0 || c == 2) return false;
            k[c++] = u;
        }
        if (c != 2) return false;
        t.kid0[(size_t)v] = std::min(k[0], k[1]); t.kid1[(size_t)v] = std::max(k[0], k[1]);
        t.par[(size_t)k[0]] = t.par[(size_t)k[1]] = v;
        t.stack.push_back(k[0]); t.stack.push_back(k[1]);
    }
    return seen == M - 1;
}

// The SPR search.  engine(tree, eval, spr_eval) evaluates a derived tree (0, or an error code that ends the search).
template <class Engine>
inline int spr_search(Tree& t, int max_rounds, Engine&& engine, Eval& cur, double* L_rounds, int64_t* stats6)
{
    Eval nxt;
    SprEval scur, snxt;
    cur.size(t.M); nxt.size(t.M); scur.size(t.M); snxt.size(t.M);
    SprMoves mv;
    std::vector<int32_t> k0, k1, pr, nb;
    derive(t);
    if (int rc = engine(t, cur, scur)) return rc;
    if (L_rounds) L_rounds[0] = cur.L;
    for (int i = 0; i < 6; ++i) stats6[i] = 0;
    for (int rounds = 0;;) {
        const int64_t cands = spr_select(t, scur, mv);
        if (rounds == 0) stats6[3] = cands;
        if (cands == 0 || rounds >= max_rounds) break;
        k0 = t.kid0; k1 = t.kid1; pr = t.par;
        const int32_t top0 = t.top;
        auto restore = [&]() { t.kid0 = k0; t.kid1 = k1; t.par = pr; t.top = top0; };
        if (!spr_apply(t, mv, 0, mv.count(), nb)) return -1;
        derive(t);
        if (int rc = engine(t, nxt, snxt)) return rc;
        size_t applied = mv.count();
        if (!(nxt.L < cur.L)) {
            ++stats6[2];
            restore();
            if (!spr_apply(t, mv, 0, 1, nb)) return -1;
            derive(t);
            if (int rc = engine(t, nxt, snxt)) return rc;
            applied = 1;
            if (!(nxt.L < cur.L)) {
                restore();
                derive(t);
                break;
            }
        }
        std::swap(cur, nxt);
        std::swap(scur, snxt);
        stats6[1] += (int64_t)applied;
        for (size_t i = 0; i < applied; ++i) {
            stats6[4] += mv.k(i) >= 2;
            stats6[5] = std::max<int64_t>(stats6[5], mv.k(i));
        }
        stats6[0] = ++rounds;
        if (L_rounds) L_rounds[rounds] = cur.L;
    }
    return 0;
}

// the host engine with the scan behind it: the table in node ids
struct SprHostEngine {
    HostEngine base;
    std::vector<int32_t> tab;
    SprTree prepare(const Tree& t)
    {
        const View w = t.view();
        for (int32_t u = 0; u < t.M; ++u) spr_mirror_w(base.T.data(), base.ld, t.M, w, u);
        tab.resize((size_t)(5 * t.M));
        spr_records(t, false, tab.data(), 4 * t.M);
        return SprTree{ base.T.data(), base.ld, reinterpret_cast<const SprRec*>(tab.data()), nullptr, nullptr, (int32_t)t.n, (int32_t)t.M, t.t0, t.top };
    }
    int operator()(const Tree& t, Eval& e, SprEval& se)
    {
        base(t, e);
        const SprTree st = prepare(t);
        for (int64_t d = 0; d < 2 * t.M; ++d) {
            SprBest b;
            spr_scan_one(st, (int32_t)d, b);
            se.gain[(size_t)d] = b.g; se.w[(size_t)d] = b.w; se.k[(size_t)d] = b.k;
        }
        return 0;
    }
};

// dpr_bme_spr_host without the library around it: 0, or -1 (bad argument / not a merge log)
inline int spr_host(const double* lower_rows, int64_t n, const int32_t* mx, const int32_t* my, int max_rounds, int32_t* kids, int32_t* top,
                    double* len, double* L_rounds, int64_t* stats6)
{
    if (!lower_rows || n < 3 || n >= ((int64_t)1 << 24) || !mx || !my || max_rounds < 0 || !kids || !top || !len || !stats6) return -1;
    Tree t;
    if (!from_merges(n, mx, my, t)) return -1;
    SprHostEngine eng;
    eng.base.fill(n, lower_rows);
    Eval cur;
    if (int rc = spr_search(t, max_rounds, eng, cur, L_rounds, stats6)) return rc;
    write_outputs(t, cur, kids, top, len);
    return 0;
}

// one scan of a given tree on the host (test hooks dpr_bme_spr_eval_host; d >= 0: dpr_bme_spr_gain_host, the gain and k of the
// target w of d alone, -2 if w is no target of d): 0, or -1
inline int spr_eval_host(const double* lower_rows, int64_t n, const int32_t* kids, int32_t top, int64_t d, int32_t w, double* gain, int32_t* bw,
                         int32_t* bk, double* L)
{
    if (!lower_rows || n < 3 || n >= ((int64_t)1 << 24) || !kids || !gain || !bk) return -1;
    Tree t;
    if (!from_kids(n, kids, top, t)) return -1;
    derive(t);
    SprHostEngine eng;
    eng.base.fill(n, lower_rows);
    Eval e;
    e.size(t.M);
    if (d >= 0) {
        if (d >= 2 * t.M || w < 0 || w >= t.M) return -2;
        eng.base(t, e);
        const SprTree st = eng.prepare(t);
        SprBest b;
        b.want = w;
        spr_scan_one(st, (int32_t)d, b);
        if (b.k == 0) return -2;
        *gain = b.g; *bk = b.k;
        return 0;
    }
    if (!bw || !L) return -1;
    SprEval se;
    se.size(t.M);
    eng(t, e, se);
    std::copy(se.gain.begin(), se.gain.end(), gain);
    std::copy(se.w.begin(), se.w.end(), bw);
    std::copy(se.k.begin(), se.k.end(), bk);
    *L = e.L;
    return 0;
}

}  // namespace bme
}  // namespace dpr
