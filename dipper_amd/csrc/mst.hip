// The minimum spanning forest of the distances (dpr_mst_run, include/dipper_hip.h; driver in ctx_mst.hip; the contract restated on the
// host in mst_host.hpp).  No reference counterpart.
//
// Boruvka: in a round every component finds its smallest outgoing edge under the contract's order (key of the distance, then the larger
// end, then the smaller); the edges found join components; the rounds end when nothing is found or one component is left.  The order is
// total, so the edges a round finds all belong to the one Kruskal forest and close no cycle (but the pair of components that chose the
// same edge, which is emitted once).
//
//   1. row minimum   mst_row_min_kernel, per block of FULL rows (row stride ld, a multiple of 16 columns; the layout nearest.hip
//      selects from).  One workgroup of kMstThreads lanes walks one row r in steps of kMstChunk columns, a lane loading two pairs of
//      neighbouring columns (16 bytes of distances and 8 bytes of labels each, both in flight).  A column counts when it is below n, its
//      label differs from the row's (the row itself never counts) and its entry is finite.  A lane meets its columns in ascending
//      order and keeps a running minimum of the key under strict <, so of equal keys the smaller column stays; within a row (key,
//      column) is the edge order.  Then a shuffle reduction on (key, column) per wave and the waves through LDS.  No atomics, no
//      candidate buffer.  The row's result is rkey / rcol and rdist, the entry's own bits re-read from the row.
//   2. component minimum   after the last block: atomicMin of rkey[r] into ckey[label[r]]; then the rows whose key is their component's
//      atomicMin (max(r, c) << 32 | min(r, c)) into cedge[label[r]].  Integer minima: the result does not depend on arrival order.  A
//      wave whose active rows share one label reduces by shuffles first and sends one atomic.
//   3. emit   one lane per component root with an edge appends it to the edge buffer (atomicAdd on the count: the place does not matter,
//      the host sorts once at the end) unless the component at the other end chose the same edge and has the smaller label.
//   4. join   the union-find of pairs.hip (pairs_hook, pairs_flatten) over the round's edges; the labels are its flattened forest.
#include "dpr_internal.hpp"

namespace dpr {

namespace {

constexpr int kMstWaves = kMstThreads / 64;
constexpr unsigned long long kMstNone = ~0ull;      // above the key of every finite distance

__device__ inline void mst_take(double v, int32_t l, int64_t c, int64_t n, int32_t mine, unsigned long long& bk, int32_t& bc)
{
    if (c >= n || l == mine || !nearest_finite(v)) return;
    const unsigned long long k = nearest_key(v);
    if (k < bk) { bk = k; bc = (int32_t)c; }
}

__global__ __launch_bounds__(kMstThreads) void mst_row_min_kernel(const double* __restrict__ rows, int64_t ld, int64_t r0, int64_t n,
                                                                   const int32_t* __restrict__ label, unsigned long long* __restrict__ rkey,
                                                                   int32_t* __restrict__ rcol, double* __restrict__ rdist)
{
    __shared__ unsigned long long wkey[kMstWaves];
    __shared__ int32_t wcol[kMstWaves];
    const int64_t r = r0 + (int64_t)blockIdx.x;
    const double* row = rows + (int64_t)blockIdx.x * ld;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t mine = label[r];
    unsigned long long bk = kMstNone;
    int32_t bc = 0x7fffffff;
    for (int64_t c0 = 0; c0 < n; c0 += kMstChunk) {
        // columns ja, ja + 1 and jb, jb + 1: ja and jb are even, as ld is, so a pair whose first column is below n lies inside the row's
        // ld columns and the labels' ld entries
        const int64_t ja = c0 + 2 * tid, jb = ja + 2 * kMstThreads;
        double2 va = make_double2(0.0, 0.0), vb = make_double2(0.0, 0.0);
        int2 la = make_int2(mine, mine), lb = make_int2(mine, mine);
        if (ja < n) { va = *reinterpret_cast<const double2*>(row + ja); la = *reinterpret_cast<const int2*>(label + ja); }
        if (jb < n) { vb = *reinterpret_cast<const double2*>(row + jb); lb = *reinterpret_cast<const int2*>(label + jb); }
        mst_take(va.x, la.x, ja, n, mine, bk, bc);
        mst_take(va.y, la.y, ja + 1, n, mine, bk, bc);
        mst_take(vb.x, lb.x, jb, n, mine, bk, bc);
        mst_take(vb.y, lb.y, jb + 1, n, mine, bk, bc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ok = __shfl_xor(bk, off);
        const int32_t oc = __shfl_xor(bc, off);
        if (ok < bk || (ok == bk && oc < bc)) { bk = ok; bc = oc; }
    }
    if (lane == 0) { wkey[wave] = bk; wcol[wave] = bc; }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < kMstWaves; ++w)
            if (wkey[w] < bk || (wkey[w] == bk && wcol[w] < bc)) { bk = wkey[w]; bc = wcol[w]; }
        const bool found = bk != kMstNone && bc >= 0 && bc < n;
        rkey[r] = found ? bk : kMstNone;
        rcol[r] = found ? bc : -1;
        rdist[r] = found ? row[bc] : __longlong_as_double(0x7ff8000000000000ll);
    }
}

// atomicMin of v into slot[l] for the lanes with `on`.  Every lane of the wave calls it.  Where the lanes that are on share one label
// the wave reduces by shuffles and its first such lane sends the one atomic
__device__ inline void mst_atomic_min(unsigned long long* slot, int32_t l, unsigned long long v, bool on, int lane)
{
    const unsigned long long act = __ballot(on);
    if (!act) return;      // (the same in every lane)
    const int first = __ffsll((long long)act) - 1;
    const int32_t l0 = __shfl(l, first);
    if (__ballot(on && l != l0) == 0) {
        unsigned long long m = on ? v : kMstNone;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(m, off);
            m = o < m ? o : m;
        }
        if (lane == first) atomicMin(slot + l0, m);
    } else if (on) {
        atomicMin(slot + l, v);
    }
}

__global__ __launch_bounds__(kMstThreads) void mst_component_key_kernel(const int32_t* __restrict__ label, const unsigned long long* __restrict__ rkey,
                                                                         int64_t n, unsigned long long* ckey)
{
    const int64_t r = (int64_t)blockIdx.x * kMstThreads + threadIdx.x;
    const int32_t l = r < n ? label[r] : -1;
    const unsigned long long k = r < n ? rkey[r] : kMstNone;
    mst_atomic_min(ckey, l, k, l >= 0 && l < n && k != kMstNone, (int)threadIdx.x & 63);
}

__global__ __launch_bounds__(kMstThreads) void mst_component_edge_kernel(const int32_t* __restrict__ label, const unsigned long long* __restrict__ rkey,
                                                                          const int32_t* __restrict__ rcol, int64_t n,
                                                                          const unsigned long long* __restrict__ ckey, unsigned long long* cedge)
{
    const int64_t r = (int64_t)blockIdx.x * kMstThreads + threadIdx.x;
    const int32_t l = r < n ? label[r] : -1;
    const unsigned long long k = r < n ? rkey[r] : kMstNone;
    const int32_t c = r < n ? rcol[r] : -1;
    const bool on = l >= 0 && l < n && c >= 0 && c < n && c != r && k != kMstNone && k == ckey[l];
    const unsigned long long hi = (unsigned long long)(r > c ? r : c), lo = (unsigned long long)(r > c ? c : r);
    mst_atomic_min(cedge, l, on ? hi << 32 | lo : kMstNone, on, (int)threadIdx.x & 63);
}

__global__ __launch_bounds__(kMstThreads) void mst_emit_kernel(const int32_t* __restrict__ label, const unsigned long long* __restrict__ cedge,
                                                                const double* __restrict__ rdist, int64_t n, int32_t* __restrict__ ei,
                                                                int32_t* __restrict__ ej, double* __restrict__ ed, int64_t cap,
                                                                unsigned long long* count)
{
    const int64_t v = (int64_t)blockIdx.x * kMstThreads + threadIdx.x;
    if (v >= n || label[v] != v) return;
    const unsigned long long e = cedge[v];
    if (e == kMstNone) return;
    const int64_t i = (int64_t)(e >> 32), j = (int64_t)(e & 0xffffffffull);
    if (i >= n || j >= i) return;      // (never: the rows' columns are below n and differ from the row)
    const int32_t li = label[i], lj = label[j];
    const int64_t row = li == v ? i : j;
    const int32_t other = li == v ? lj : li;
    if (other < 0 || other >= n || other == v) return;      // (never: an edge leaves its component)
    if (cedge[other] == e && other < v) return;             // both ends chose it: the smaller label emits
    const unsigned long long at = atomicAdd(count, 1ull);
    if (at < (unsigned long long)cap) { ei[at] = (int32_t)i; ej[at] = (int32_t)j; ed[at] = rdist[row]; }      // (a count beyond cap is the host's error)
}

inline unsigned mst_grid(int64_t items) { return (unsigned)((items + kMstThreads - 1) / kMstThreads); }

}  // namespace

int mst_row_min(const double* rows, int64_t ld, int64_t r0, int64_t nr, int64_t n, const int32_t* label, unsigned long long* rkey,
                int32_t* rcol, double* rdist, hipStream_t s)
{
    if (nr < 1 || nr > kPairsMaxRows || n < 2 || r0 < 0 || r0 + nr > n || ld < n || ld % 2) { set_error("mst_row_min: a block out of range"); return DPR_ERR_ARG; }
    hipLaunchKernelGGL(mst_row_min_kernel, dim3((unsigned)nr), dim3(kMstThreads), 0, s, rows, ld, r0, n, label, rkey, rcol, rdist);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

int mst_component_min_emit(const int32_t* label, const unsigned long long* rkey, const int32_t* rcol, const double* rdist, int64_t n,
                           unsigned long long* ckey, unsigned long long* cedge, int32_t* ei, int32_t* ej, double* ed, int64_t cap,
                           unsigned long long* count, hipStream_t s)
{
    if (n < 2 || cap < 1) { set_error("mst_component_min_emit: out of range"); return DPR_ERR_ARG; }
    DPR_HIP(hipMemsetAsync(ckey, 0xff, sizeof(unsigned long long) * (size_t)n, s));
    DPR_HIP(hipMemsetAsync(cedge, 0xff, sizeof(unsigned long long) * (size_t)n, s));
    hipLaunchKernelGGL(mst_component_key_kernel, dim3(mst_grid(n)), dim3(kMstThreads), 0, s, label, rkey, n, ckey);
    DPR_HIP(hipGetLastError());
    hipLaunchKernelGGL(mst_component_edge_kernel, dim3(mst_grid(n)), dim3(kMstThreads), 0, s, label, rkey, rcol, n, (const unsigned long long*)ckey, cedge);
    DPR_HIP(hipGetLastError());
    hipLaunchKernelGGL(mst_emit_kernel, dim3(mst_grid(n)), dim3(kMstThreads), 0, s, label, (const unsigned long long*)cedge, rdist, n, ei, ej, ed, cap, count);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

}  // namespace dpr
