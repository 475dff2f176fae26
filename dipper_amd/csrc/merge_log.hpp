// Merge logs of dpr_nj_run (NJ, BIONJ: n - 2 entries) and dpr_upgma_run (n - 1 entries), replayed in one place.  Plain C++17, std
// only: the library, the stand-alone check drivers and the command include it.
//
// A log names SLOTS, not nodes.  Slots 0 .. n-1 start out holding tips 0 .. n-1.  Merge `it` finds n - it live slots, joins the
// nodes in slots x and y into node n + it, leaves that node in slot x and moves the last live slot into y (the realID bookkeeping
// of the reference, src/neighborJoining.cu:233-237).  After an NJ log two slots are left: the root 2n - 2 joins their nodes.
//
// Two rules say what a log entry may be:
//   strict    0 <= x < y < n - it            what dpr_nj_run and dpr_upgma_run emit
//   lenient   0 <= x, y < n - it, x != y     what dpr_tree_from_nj and dpr_tree_from_upgma accept
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace merge_log {

// the slot move of one merge over `live` slots: `node` stays in x, the last live slot moves into y (nothing moves when y is the last)
inline void join_slots(int32_t* real, int64_t x, int64_t y, int64_t live, int32_t node)
{
    real[x] = node;
    real[y] = real[live - 1];
}

// Replays merges [0, count), count <= n - 1: join(it, node, u, v) with node = n + it and u, v the nodes in slots x, y, before the
// slot move.  false at the first entry that breaks the rule (join has run for the entries before it).  Afterwards real[0 .. n - count)
// holds the nodes of the live slots: real[0], real[1] are the pair the NJ root joins.
template <bool kStrict, class Join>
inline bool replay(int64_t n, int64_t count, const int32_t* mx, const int32_t* my, std::vector<int32_t>& real, Join&& join)
{
    real.resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) real[(size_t)i] = (int32_t)i;
    for (int64_t it = 0; it < count; ++it) {
        const int64_t x = mx[it], y = my[it], live = n - it;
        if (kStrict ? (x < 0 || y <= x || y >= live) : (x < 0 || y < 0 || x >= live || y >= live || x == y)) return false;
        const int32_t node = (int32_t)(n + it);
        join(it, node, real[(size_t)x], real[(size_t)y]);
        join_slots(real.data(), x, y, live, node);
    }
    return true;
}

// The rooted tree the command writes for an NJ / BIONJ log: edge(parent, side, child, len) for every edge, side 0 the x child on
// bx[it], side 1 the y child on by[it]; the root 2n - 2 holds the two nodes left, EACH on half of `last`.  n >= 2.
template <bool kStrict, class Edge>
inline bool nj_edges(int64_t n, const int32_t* mx, const int32_t* my, const double* bx, const double* by, double last, Edge&& edge)
{
    std::vector<int32_t> real;
    auto join = [&](int64_t it, int32_t node, int32_t u, int32_t v) { edge(node, 0, u, bx[it]); edge(node, 1, v, by[it]); };
    if (!replay<kStrict>(n, n - 2, mx, my, real, join)) return false;
    const int32_t root = (int32_t)(2 * n - 2);
    edge(root, 0, real[0], last * 0.5);
    edge(root, 1, real[1], last * 0.5);
    return true;
}

// The same for a UPGMA / WPGMA log of n - 1 merges, the last one the root: a branch is height[it] - h(child), h of a tip 0.0 and of
// internal node u height[u - n].
template <bool kStrict, class Edge>
inline bool upgma_edges(int64_t n, const int32_t* mx, const int32_t* my, const double* height, Edge&& edge)
{
    std::vector<int32_t> real;
    auto h = [&](int32_t u) { return u < n ? 0.0 : height[u - n]; };
    auto join = [&](int64_t it, int32_t node, int32_t u, int32_t v) { edge(node, 0, u, height[it] - h(u)); edge(node, 1, v, height[it] - h(v)); };
    return replay<kStrict>(n, n - 1, mx, my, real, join);
}

// Clade sizes and children of an NJ log: size[v] tips below node v < 2n - 2; kid[2 it], kid[2 it + 1] the x and y child of node
// n + it; root[] the pair the root joins.
struct Sizes {
    std::vector<int32_t> size, kid;
    int32_t root[2] = { 0, 1 };
};
template <bool kStrict>
inline bool sizes_of(int64_t n, const int32_t* mx, const int32_t* my, Sizes& s)
{
    s.size.assign((size_t)(2 * n - 2), 1);
    s.kid.assign((size_t)(2 * (n - 2)), 0);
    std::vector<int32_t> real;
    auto join = [&](int64_t it, int32_t node, int32_t u, int32_t v) {
        s.kid[(size_t)(2 * it)] = u; s.kid[(size_t)(2 * it + 1)] = v;
        s.size[(size_t)node] = s.size[(size_t)u] + s.size[(size_t)v];
    };
    if (!replay<kStrict>(n, n - 2, mx, my, real, join)) return false;
    s.root[0] = real[0]; s.root[1] = real[1];
    return true;
}

}  // namespace merge_log
