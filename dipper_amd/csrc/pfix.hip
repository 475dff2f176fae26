// Independent placement of queries on a fixed backbone on gfx950 (no reference counterpart: the reference's addQuery,
// src/placement_close_k.cu:858-990, inserts the queries one after the other; findClustersDC, src/divide_and_conquer/
// placement_close_k.cu:937-1113, scores them independently but keeps the edge only).
//
// Per query q and eligible slot s (belong >= e, one per undirected edge) the arithmetic of calculateBranchLength
// (src/placement_close_k.cu:309-358) gives the pendant length `add` and the position `frac` (distance of the attachment point
// from node belong[s]); the placement of q is the slot with the smallest (add, slot).  The scan is the divide-and-conquer
// assignment's (dc_scan.hpp: a lane is a query, the edge is wave-uniform, a chunk's distance rows and records in LDS).  The position
// of the winner comes from one of two forms that give the same bits:
//   re-evaluate (default)  the scan is the assignment's own, minima only; the reduce step evaluates the winning entry once
//                          more from the table and the batch's distance block (ten loads per QUERY);
//   carry                  the scan carries the position with its running minimum (the `rest / 2` step on every EDGE, a third
//                          array of per-chunk partials).
// Measurements of both: DESIGN.md section 11.
#include "dc_scan.hpp"

namespace dpr {

template <bool kCarry>
__global__ __launch_bounds__(256) void pfix_scan_kernel(const int32_t* __restrict__ ch_e0, const int32_t* __restrict__ ch_l0,
                                                        const int32_t* __restrict__ ch_leaf, const uint4* __restrict__ et_rec,
                                                        const double* __restrict__ dT, int64_t ldq, int Q,
                                                        double* __restrict__ part_add, int32_t* __restrict__ part_pos,
                                                        double* __restrict__ part_frac)
{
    dc_scan_chunk<kCarry>(ch_e0, ch_l0, ch_leaf, et_rec, dT, ldq, Q, part_add, part_pos, part_frac);
}

// minimum over the chunks in the (add, slot) order; 64 queries per workgroup, its 16 wavefronts every 16th chunk (as
// dc_assign_reduce_kernel).  !kCarry: the winning entry is evaluated again -- the scan's operations in the scan's order on the
// same numbers (an absent list entry is skipped where the scan reads its row of -inf: fmax leaves the maximum alone either way).
constexpr int kPfRedWaves = 16;
template <bool kCarry>
__global__ __launch_bounds__(64 * kPfRedWaves) void pfix_reduce_kernel(const double* __restrict__ part_add, const int32_t* __restrict__ part_pos,
                                                                       const double* __restrict__ part_frac, int nchunks, int64_t ldq, int Q,
                                                                       const double* __restrict__ dT, const int32_t* __restrict__ ent_of_slot,
                                                                       int nslots, const int32_t* __restrict__ et_cid,
                                                                       const double* __restrict__ et_cdis, const double* __restrict__ et_len,
                                                                       int32_t* __restrict__ out_slot, double* __restrict__ out_frac,
                                                                       double* __restrict__ out_add)
{
    __shared__ double s_best[kPfRedWaves][64];
    __shared__ int s_pos[kPfRedWaves][64];
    __shared__ double s_frac[kCarry ? kPfRedWaves : 1][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = blockIdx.x * 64 + lane;
    const int qq = q < Q ? q : Q - 1;
    double best = __builtin_inf(), bfrac = 0;
    int bpos = 0x7fffffff;
#pragma unroll 4
    for (int c = w; c < nchunks; c += kPfRedWaves) {
        const double a = part_add[(int64_t)c * ldq + qq];
        const int sl = part_pos[(int64_t)c * ldq + qq];
        if (a < best || (a == best && sl < bpos)) { best = a; bpos = sl; if (kCarry) bfrac = part_frac[(int64_t)c * ldq + qq]; }
    }
    s_best[w][lane] = best; s_pos[w][lane] = bpos;
    if (kCarry) s_frac[w][lane] = bfrac;
    __syncthreads();
    if (w == 0 && q < Q) {
#pragma unroll
        for (int k = 1; k < kPfRedWaves; ++k) {
            const double a = s_best[k][lane];
            const int sl = s_pos[k][lane];
            if (a < best || (a == best && sl < bpos)) { best = a; bpos = sl; if (kCarry) bfrac = s_frac[k][lane]; }
        }
        const bool found = bpos >= 0 && bpos < nslots;      // (always: the table has an entry and no pendant length is a NaN)
        const int e = !kCarry && found ? ent_of_slot[bpos] : -1;
        if (e >= 0) {
            const double* col = dT + q;
            double dis1 = 0, dis2 = 0;
#pragma unroll
            for (int i = 0; i < K5; ++i) {
                const int id = et_cid[e * 10 + i];
                if (id >= 0) dis1 = fmax(dis1, col[(int64_t)id * ldq] - et_cdis[e * 10 + i]);
            }
#pragma unroll
            for (int i = 0; i < K5; ++i) {
                const int id = et_cid[e * 10 + 5 + i];
                if (id >= 0) dis2 = fmax(dis2, col[(int64_t)id * ldq] - et_cdis[e * 10 + 5 + i]);
            }
            const double L = et_len[e];
            double a = (dis1 + dis2 - L) / 2;
            if (a < 0) a = 0;
            dis1 -= a; dis2 -= a;
            if (dis1 < 0) dis1 = 0;
            if (dis2 < 0) dis2 = 0;
            if (dis1 > L) { a += dis1 - L; dis1 = L; }
            if (dis2 > L) { a += dis2 - L; dis2 = L; }
            const double rest = L - dis1 - dis2;
            dis1 += rest / 2;
            bfrac = dis1;
        }
        out_slot[q] = found ? bpos : -1;
        out_frac[q] = found ? bfrac : 0.0;
        out_add[q] = best;
    }
}

__global__ __launch_bounds__(kThreads) void pfix_entry_of_slot_kernel(const int32_t* __restrict__ vslots, int nv, int nslots,
                                                                      int32_t* __restrict__ ent_of_slot)
{
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e >= nv) return;
    const int s = vslots[e];
    if (s >= 0 && s < nslots) ent_of_slot[s] = e;
}

int pfix_set(PlaceFixed& f, PlaceBuffers& p, int64_t m, hipStream_t s)
{
    f.valid = false;
    if (int rc = dc_table_build(p, m, f.tab, s)) return rc;
    const int64_t nslots = 4 * m - 4;
    if (f.ent_of_slot) { (void)hipFree(f.ent_of_slot); f.ent_of_slot = nullptr; }
    DPR_HIP(hipMalloc(&f.ent_of_slot, sizeof(int32_t) * (size_t)nslots));
    DPR_HIP(hipMemsetAsync(f.ent_of_slot, 0xff, sizeof(int32_t) * (size_t)nslots, s));
    hipLaunchKernelGGL(pfix_entry_of_slot_kernel, dim3((unsigned)((f.tab.nv + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, f.tab.vslots,
                       f.tab.nv, (int)nslots, f.ent_of_slot);
    DPR_HIP(hipGetLastError());
    f.m = m;
    f.n = p.N;
    f.valid = true;
    return DPR_OK;
}

void pfix_free(PlaceFixed& f)
{
    dc_table_free(f.tab);
    void* ptrs[] = { f.ent_of_slot, f.part_frac, f.dT, f.slot, f.frac, f.add };
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
    const int64_t batch = f.batch;      // (the hook belongs to the context, not to a backbone)
    f = PlaceFixed();
    f.batch = batch;
}

int pfix_place(PlaceFixed& f, const double* dT, int64_t ldq, int Q, int32_t* d_slot, double* d_frac, double* d_add, bool carry,
               hipStream_t s)
{
    DcTable& t = f.tab;
    if (int rc = dc_parts_reserve(t, ldq)) return rc;
    const size_t need = (size_t)t.nch * (size_t)ldq;
    if (carry && need > f.part_frac_cap) {
        if (f.part_frac) { (void)hipFree(f.part_frac); f.part_frac = nullptr; f.part_frac_cap = 0; }
        DPR_HIP(hipMalloc(&f.part_frac, sizeof(double) * need));
        f.part_frac_cap = need;
    }
    // chunks are the fast grid index, as in dc_assign: the blocks in flight share few query groups
    const dim3 grid((unsigned)t.nch, (unsigned)((Q + 63) / 64)), rgrid((unsigned)((Q + 63) / 64));
    const int nslots = (int)(4 * f.m - 4);
    if (carry) {
        hipLaunchKernelGGL(pfix_scan_kernel<true>, grid, dim3(256), 0, s, t.ch_e0, t.ch_l0, t.ch_leaf, t.et_rec, dT, ldq, Q, t.part_add,
                           t.part_pos, f.part_frac);
        hipLaunchKernelGGL(pfix_reduce_kernel<true>, rgrid, dim3(64 * kPfRedWaves), 0, s, t.part_add, t.part_pos, f.part_frac, t.nch, ldq, Q,
                           dT, f.ent_of_slot, nslots, t.et_cid, t.et_cdis, t.et_len, d_slot, d_frac, d_add);
    } else {
        hipLaunchKernelGGL(pfix_scan_kernel<false>, grid, dim3(256), 0, s, t.ch_e0, t.ch_l0, t.ch_leaf, t.et_rec, dT, ldq, Q, t.part_add,
                           t.part_pos, (double*)nullptr);
        hipLaunchKernelGGL(pfix_reduce_kernel<false>, rgrid, dim3(64 * kPfRedWaves), 0, s, t.part_add, t.part_pos, (const double*)nullptr,
                           t.nch, ldq, Q, dT, f.ent_of_slot, nslots, t.et_cid, t.et_cdis, t.et_len, d_slot, d_frac, d_add);
    }
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

}  // namespace dpr
