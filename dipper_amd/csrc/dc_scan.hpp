// The chunked edge scan of a frozen backbone, shared by the divide-and-conquer cluster assignment (dc.hip) and the
// fixed-backbone placement (pfix.hip): chunk layout of DcTable and the scan of one (chunk, 64 queries) workgroup.
#pragma once
#include "dpr_internal.hpp"

namespace dpr {

constexpr int K5 = 5;
constexpr int kAE = 64;       // backbone edges per scan chunk at most (their records sit in LDS: 176 B each)
constexpr int kDcRows = 48;   // distinct closest leaves per chunk = distance rows staged in LDS (64 queries x 8 B each) + one row of -inf
constexpr int kDcRec = 11;    // 16-byte words per packed table entry

// calculateBranchLengthDC for (chunk of table entries blockIdx.x) x (64 queries blockIdx.y); lane = query.
// dT[c * ldq + q] = distance(query q, backbone tip c).  Writes the chunk's first minimum per query.
// One workgroup = 64 queries x one chunk of table entries.  Round 5: the chunk's distinct closest leaves (<= kDcRows; neighbours in
// the tree share most of theirs: 47 rows for 56 entries' 560 references on average) are staged in LDS once -- a lane per query,
// the four wavefronts a quarter of the rows each, all loads in flight together -- and the 10 look-ups per entry read LDS at a
// wave-uniform row; the former scan read every reference from L2 / Infinity Cache (7.6 TB per 950 000 queries x 100 000 edges,
// 3.5 ms per launch).  The four wavefronts then take every fourth entry of the chunk for the same 64 queries and combine their
// minima.  The entries' scalars (row offset and path length per list entry, edge length, slot) are copied to LDS with the rows and
// read there at a wave-uniform address (a broadcast): as scalar loads they shared a counter with the LDS reads and made every
// entry a chain of five dependent round trips (2.3 ms); as one record per entry read out with v_readlane they were a third of
// the loop's vector instructions (1.4 ms).  An absent list entry points at a row of -inf: its candidate never exceeds the running
// maximum, as the reference's `!= -1` test.  Same arithmetic per (query, edge); the minimum does not depend on the order (ties
// by slot).
// kFrac: the position on the edge (distance of the attachment point from belong[slot]) is carried with the minimum and written
// to part_frac -- the `rest / 2` step on every edge; without it part_frac is not touched.
template <bool kFrac>
__device__ __forceinline__ void dc_scan_chunk(const int32_t* __restrict__ ch_e0, const int32_t* __restrict__ ch_l0,
                                              const int32_t* __restrict__ ch_leaf, const uint4* __restrict__ et_rec,
                                              const double* __restrict__ dT, int64_t ldq, int Q, double* __restrict__ part_add,
                                              int32_t* __restrict__ part_pos, double* __restrict__ part_frac)
{
    __shared__ double rows[(kDcRows + 1) * 64];
    __shared__ uint4 meta[kAE * kDcRec];
    __shared__ double s_best[3][64];
    __shared__ int s_pos[3][64];
    __shared__ double s_frac[kFrac ? 3 : 1][64];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int ch = blockIdx.x;
    const int q = blockIdx.y * 64 + lane;
    const int qq = q < Q ? q : Q - 1;
    const int e0 = ch_e0[ch], e1 = ch_e0[ch + 1], l0 = ch_l0[ch], nrow = ch_l0[ch + 1] - l0;
    const double* col = dT + qq;
    {
        const int nm = (e1 - e0) * kDcRec;
        const uint4* __restrict__ src = et_rec + (int64_t)e0 * kDcRec;
        uint4 m[(kAE * kDcRec + 255) / 256];
#pragma unroll
        for (int k = 0; k < (kAE * kDcRec + 255) / 256; ++k) {
            const int idx = (int)threadIdx.x + 256 * k;
            m[k] = idx < nm ? src[idx] : make_uint4(0u, 0u, 0u, 0u);
        }
        double v[kDcRows / 4];
#pragma unroll
        for (int k = 0; k < kDcRows / 4; ++k) {
            const int r = w + 4 * k;
            v[k] = r < nrow ? col[(int64_t)ch_leaf[l0 + r] * ldq] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < (kAE * kDcRec + 255) / 256; ++k) {
            const int idx = (int)threadIdx.x + 256 * k;
            if (idx < nm) meta[idx] = m[k];
        }
#pragma unroll
        for (int k = 0; k < kDcRows / 4; ++k) {
            const int r = w + 4 * k;
            if (r < nrow) rows[r * 64 + lane] = v[k];
        }
        if (w == 0) rows[kDcRows * 64 + lane] = -__builtin_inf();
    }
    __syncthreads();
    double best = __builtin_inf(), bfrac = 0;
    int bpos = 0x7fffffff;      // the SLOT of the best edge: ties go to the lowest slot
    auto f64_of = [](const uint4& u) -> double { return __longlong_as_double((long long)(((unsigned long long)u.w << 32) | u.z)); };
    const int ne = e1 - e0;
#pragma unroll 2
    for (int el = w; el < ne; el += 4) {
        const uint4* __restrict__ mr = meta + el * kDcRec;
        // (fmax for the reference's `if (val > dis) dis = val`: dis starts at +0 and only ever takes a larger value, a NaN candidate is
        //  passed over by both forms)
        double dis1 = 0, dis2 = 0;
#pragma unroll
        for (int i = 0; i < K5; ++i) { const uint4 u = mr[i]; dis1 = fmax(dis1, rows[u.x + lane] - f64_of(u)); }
#pragma unroll
        for (int i = 0; i < K5; ++i) { const uint4 u = mr[5 + i]; dis2 = fmax(dis2, rows[u.x + lane] - f64_of(u)); }
        const uint4 t = mr[10];
        const double L = f64_of(t);
        double a = (dis1 + dis2 - L) / 2;
        if (a < 0) a = 0;
        dis1 -= a; dis2 -= a;
        if (dis1 < 0) dis1 = 0;
        if (dis2 < 0) dis2 = 0;
        if (dis1 > L) { a += dis1 - L; dis1 = L; }
        if (dis2 > L) { a += dis2 - L; dis2 = L; }
        const int slot = (int)t.x;
        if (kFrac) {
            const double rest = L - dis1 - dis2;
            dis1 += rest / 2;
        }
        if (a < best || (a == best && slot < bpos)) { best = a; bpos = slot; if (kFrac) bfrac = dis1; }
    }
    if (w > 0) { s_best[w - 1][lane] = best; s_pos[w - 1][lane] = bpos; if (kFrac) s_frac[w - 1][lane] = bfrac; }
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double a = s_best[k][lane];
            const int sl = s_pos[k][lane];
            if (a < best || (a == best && sl < bpos)) { best = a; bpos = sl; if (kFrac) bfrac = s_frac[k][lane]; }
        }
        if (q < Q) {
            part_add[(int64_t)blockIdx.x * ldq + q] = best;
            part_pos[(int64_t)blockIdx.x * ldq + q] = bpos;
            if (kFrac) part_frac[(int64_t)blockIdx.x * ldq + q] = bfrac;
        }
    }
}

}  // namespace dpr
