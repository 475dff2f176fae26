// The minimum spanning forest of the distances and its single-linkage dendrogram, restated on the host: plain C++, no HIP
// (include/dipper_hip.h, dpr_mst_host, dpr_mst_dendrogram_host).  Kruskal: every finite entry of the strict lower triangle is a
// candidate, the candidates are sorted under the contract's order (key of the distance, then i, then j) and a union-find that hangs the
// larger root under the smaller takes an edge whenever its ends are not joined yet -- on purpose not the device's algorithm (Boruvka
// rounds over streamed row blocks; mst.hip), which must reproduce it edge for edge and bit for bit.  Shared by the library (the host
// entry points, the order and the check of the device's edges) and mst_check.cpp (`make mst_asan`).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace mst {

inline uint64_t bits_of(double d)
{
    uint64_t b;
    std::memcpy(&b, &d, sizeof b);
    return b;
}

// the key of nearest.hip: the bits of d (of +0.0 for either zero), the sign bit flipped for d >= 0 and all bits flipped for d < 0;
// unsigned order of the keys = order of the finite distances
inline uint64_t key_of(double d)
{
    const uint64_t b = d == 0.0 ? 0ull : bits_of(d);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}

struct Edge { uint64_t key; int32_t i, j; double d; };

inline bool before(const Edge& a, const Edge& b) { return a.key != b.key ? a.key < b.key : a.i != b.i ? a.i < b.i : a.j < b.j; }

inline int32_t find_root(const std::vector<int32_t>& parent, int32_t v)
{
    while (parent[(size_t)v] != v) v = parent[(size_t)v];
    return v;
}

// joins the components of a and b (the larger root under the smaller); false when they are one already
inline bool join(std::vector<int32_t>& parent, int32_t a, int32_t b)
{
    const int32_t ra = find_root(parent, a), rb = find_root(parent, b);
    if (ra == rb) return false;
    parent[(size_t)(ra > rb ? ra : rb)] = ra > rb ? rb : ra;
    return true;
}

// The E edges of a forest over n tips (i > j, d the entry's bits), in any order -> the contract's order in place, and label[v] = the
// smallest index of v's component.  Returns 0; -1 when an edge is out of range or not finite, or joins two tips that smaller edges
// joined already (the edges are no forest).
inline int order_and_label(int64_t n, int32_t* ei, int32_t* ej, double* ed, int64_t E, int32_t* label)
{
    if (n < 1 || E < 0 || E > n - 1) return -1;
    std::vector<Edge> e((size_t)E);
    for (int64_t t = 0; t < E; ++t) {
        if (ej[t] < 0 || ei[t] <= ej[t] || ei[t] >= n || !std::isfinite(ed[t])) return -1;
        e[(size_t)t] = Edge{ key_of(ed[t]), ei[t], ej[t], ed[t] };
    }
    std::sort(e.begin(), e.end(), before);
    std::vector<int32_t> parent((size_t)n);
    for (int64_t v = 0; v < n; ++v) parent[(size_t)v] = (int32_t)v;
    for (const Edge& x : e)
        if (!join(parent, x.i, x.j)) return -1;
    for (int64_t t = 0; t < E; ++t) { ei[t] = e[(size_t)t].i; ej[t] = e[(size_t)t].j; ed[t] = e[(size_t)t].d; }
    for (int64_t v = 0; v < n; ++v) label[(size_t)v] = find_root(parent, (int32_t)v);
    return 0;
}

// lower_rows: the strict lower triangle row by row (row i holds i entries).  The Kruskal forest under the order: its edges ascending
// in ei / ej / ed (n - 1 places each), *edges their number, label[n].  Returns 0, or -1 for a bad argument (nothing is written then).
inline int mst_host(const double* lower_rows, int64_t n, int32_t* ei, int32_t* ej, double* ed, int64_t* edges, int32_t* label)
{
    if (!lower_rows || n < 2 || n >= ((int64_t)1 << 31) || !ei || !ej || !ed || !edges || !label) return -1;
    std::vector<Edge> cand;
    cand.reserve((size_t)(n * (n - 1) / 2));
    const double* row = lower_rows;
    for (int64_t a = 1; a < n; ++a) {
        row += a - 1;
        for (int64_t b = 0; b < a; ++b)
            if (std::isfinite(row[b])) cand.push_back(Edge{ key_of(row[b]), (int32_t)a, (int32_t)b, row[b] });
    }
    std::sort(cand.begin(), cand.end(), before);
    std::vector<int32_t> parent((size_t)n);
    for (int64_t v = 0; v < n; ++v) parent[(size_t)v] = (int32_t)v;
    int64_t E = 0;
    for (const Edge& x : cand) {
        if (!join(parent, x.i, x.j)) continue;
        ei[E] = x.i; ej[E] = x.j; ed[E] = x.d;
        if (++E == n - 1) break;
    }
    *edges = E;
    for (int64_t v = 0; v < n; ++v) label[(size_t)v] = find_root(parent, (int32_t)v);
    return 0;
}

// The single-linkage dendrogram of a CONNECTED forest (edges == n - 1, in the contract's order) as a merge log in the slot convention
// of dpr_upgma_run (merge_log.hpp): merge t joins the components of edge t into node n + t at height 0.5 * ed[t]; the node stays in
// the smaller of the two slots, the last live slot moves into the other.  n - 1 entries each.  Returns 0, or -1 for a bad argument or
// edges that do not span the tips (nothing meaningful is written then).
inline int dendrogram_host(int64_t n, const int32_t* ei, const int32_t* ej, const double* ed, int64_t edges, int32_t* mx, int32_t* my,
                           double* height)
{
    if (n < 2 || n >= ((int64_t)1 << 31) || edges != n - 1 || !ei || !ej || !ed || !mx || !my || !height) return -1;
    for (int64_t t = 0; t < edges; ++t)
        if (ej[t] < 0 || ei[t] <= ej[t] || ei[t] >= n) return -1;
    std::vector<int32_t> parent((size_t)n), slot_of((size_t)n), root_in((size_t)n);      // slot of a component's root; root in a slot
    for (int64_t v = 0; v < n; ++v) parent[(size_t)v] = slot_of[(size_t)v] = root_in[(size_t)v] = (int32_t)v;
    std::vector<int32_t> lx((size_t)edges), ly((size_t)edges);
    for (int64_t t = 0; t < edges; ++t) {
        const int32_t ra = find_root(parent, ei[t]), rb = find_root(parent, ej[t]);
        if (ra == rb) return -1;
        const int32_t sa = slot_of[(size_t)ra], sb = slot_of[(size_t)rb];
        const int32_t x = sa < sb ? sa : sb, y = sa < sb ? sb : sa, last = (int32_t)(n - t - 1);
        const int32_t r = ra < rb ? ra : rb;
        parent[(size_t)(ra < rb ? rb : ra)] = r;
        slot_of[(size_t)r] = x; root_in[(size_t)x] = r;
        if (y != last) { const int32_t moved = root_in[(size_t)last]; root_in[(size_t)y] = moved; slot_of[(size_t)moved] = y; }
        lx[(size_t)t] = x; ly[(size_t)t] = y;
    }
    for (int64_t t = 0; t < edges; ++t) { mx[t] = lx[(size_t)t]; my[t] = ly[(size_t)t]; height[t] = 0.5 * ed[t]; }
    return 0;
}

}  // namespace mst
