// Balanced minimum evolution (Desper & Gascuel 2002; no reference counterpart: the reference stops at the NJ tree): NNI search
// from the tree of a merge log, and the balanced branch lengths of the tree it ends on.  Contract: include/dipper_hip.h above
// dpr_bme_nni.  bme_host.hpp holds what the host and the device share -- the tree, the selection, the search loop and the per-node
// arithmetic -- and the host engine of dpr_bme_nni_host; here are the device engine and the entry points.
//
// One evaluation of a tree on the device (table T over the M = 2n - 2 nodes, see bme_host.hpp):
//   fill     once per call: tip against tip from the context's fresh matrix, always its lower triangle (both orientations of T
//            get the same bits);
//   S rows   T is indexed by a node's place in rank order (tips keep their ids, the internal nodes follow by (height, id)), so the
//            nodes of one height are neighbouring rows and everything of smaller height lies before them.  Per height h, ascending:
//            pass 1, the batch's rows against all columns before the batch and outside the row's clade, T[u][v] = 0.5 (T[c0(u)][v] +
//            T[c1(u)][v]) -- two finished rows read coalesced -- and the same value into T[v][u], transposed through LDS so that
//            both stores are runs of neighbours; pass 2, the pairs inside the batch, the later place taking the average: it reads
//            what pass 1 mirrored.  Two launches per height: 2 log2 n for a balanced tree, n - 2 small ones for a caterpillar (one
//            row per height, no pass 2; a few microseconds of launch each).  The places change from round to round with the heights;
//            every element that is read is rebuilt in the same evaluation, the tip block never moves;
//   W        one thread per node walks from the top node down to its parent (the child on the way is the one whose pre-order
//            interval holds the node) and carries W in a register: one launch, sum of the depths steps;
//   lengths  one thread per node: the length of the edge above it, its two gains and its candidate move.
// The host then sums L, selects and applies the moves (O(n)) and uploads the new tree: 36 M bytes up, 20 M bytes down a round.
#include "ctx_internal.hpp"

#include "bme_host.hpp"

namespace dpr {

namespace {

constexpr int kItabArrays = 9;      // kid0, kid1, par, sib, height, tin, tout, rows, pos
constexpr int kTileRows = 32, kTileCols = 64;      // tile of bme_s_kernel

__device__ inline bme::View bme_view(const int32_t* itab, int64_t ldi, int32_t t0, int32_t top)
{
    return bme::View{ itab, itab + ldi, itab + 2 * ldi, itab + 3 * ldi, itab + 4 * ldi, itab + 5 * ldi, itab + 6 * ldi, t0, top, itab + 8 * ldi };
}

// T[i][j] = matrix entry of the pair {i, j}, read at (max, min).  src: the context's matrix, row stride sld; pos: position of
// every slot when the matrix lives in position space, else null.  One block: 256 columns of one row.
__global__ __launch_bounds__(kThreads) void bme_fill_kernel(double* __restrict__ T, int64_t ld, int64_t n, const double* __restrict__ src,
                                                            int64_t sld, const int32_t* __restrict__ pos, int64_t colblocks)
{
    const int64_t i = blockIdx.x / colblocks, j = (blockIdx.x % colblocks) * kThreads + threadIdx.x;
    if (i >= n || j >= n || i == j) return;
    int64_t hi = i > j ? i : j, lo = i > j ? j : i;
    if (pos) { hi = pos[hi]; lo = pos[lo]; }
    T[i * ld + j] = src[hi * sld + lo];
}

// The rows of one height are the places [r0, r0 + count) of T.  kSame = false: against the columns [0, r0) -- every node of smaller
// height -- outside the row's clade; true: against the columns of the same height at a smaller place.  One block: a tile of 32 rows
// x 64 columns; the values go to T[row][column] as they are computed (64 neighbours a store) and, through LDS, to T[column][row]
// (32 neighbours a store).  Nothing a launch reads is written by it: it reads rows below r0 at columns below r0 (kSame: at the
// batch's columns, which the other pass has written) and writes rows from r0 on, and rows below r0 at columns from r0 on.
template <bool kSame>
__global__ __launch_bounds__(kThreads) void bme_s_kernel(double* __restrict__ T, int64_t ld, int64_t n, const int32_t* __restrict__ itab,
                                                         int64_t ldi, int64_t r0, int64_t count, int64_t colblocks)
{
    __shared__ double s_val[kTileRows][kTileCols + 1];
    __shared__ unsigned char s_ok[kTileRows][kTileCols + 1];
    const int64_t rbase = r0 + (blockIdx.x / colblocks) * kTileRows, rend = r0 + count;
    const int64_t cbase = (kSame ? r0 : 0) + (blockIdx.x % colblocks) * kTileCols, cend = kSame ? rend : r0;
    const int32_t* rows = itab + 7 * ldi;
    const int32_t* tin = itab + 5 * ldi;
    const int32_t* tout = itab + 6 * ldi;
    const int32_t* pos = itab + 8 * ldi;
    {
        const int c = threadIdx.x % kTileCols;
        const int64_t cp = cbase + c;
        const int32_t v = cp < cend ? (cp < n ? (int32_t)cp : rows[cp - n]) : -1;
        const int32_t tv = v >= 0 ? tin[v] : 0;
        for (int r = threadIdx.x / kTileCols; r < kTileRows; r += kThreads / kTileCols) {
            const int64_t rp = rbase + r;
            bool ok = rp < rend && v >= 0;
            double val = 0.0;
            if (ok) {
                const int32_t u = rows[rp - n];
                ok = kSame ? cp < rp : !(tin[u] <= tv && tv < tout[u]);
                if (ok) {
                    const int64_t a = pos[itab[u]], b = pos[itab[ldi + u]];
                    val = bme::avg2(T[a * ld + cp], T[b * ld + cp]);
                    T[rp * ld + cp] = val;
                }
            }
            s_val[r][c] = val;
            s_ok[r][c] = ok;
        }
    }
    __syncthreads();
    {
        const int r = threadIdx.x % kTileRows;
        for (int c = threadIdx.x / kTileRows; c < kTileCols; c += kThreads / kTileRows)
            if (s_ok[r][c]) T[(cbase + c) * ld + rbase + r] = s_val[r][c];
    }
}

__global__ __launch_bounds__(kThreads) void bme_w_kernel(double* __restrict__ T, int64_t ld, int64_t M, const int32_t* __restrict__ itab,
                                                         int64_t ldi, int32_t t0, int32_t top)
{
    const int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (u >= M) return;
    bme::walk_w(T, ld, M, bme_view(itab, ldi, t0, top), (int32_t)u);
}

__global__ __launch_bounds__(kThreads) void bme_len_kernel(const double* __restrict__ T, int64_t ld, int64_t M, const int32_t* __restrict__ itab,
                                                           int64_t ldi, int32_t t0, int32_t top, double* __restrict__ out,
                                                           int32_t* __restrict__ omove)
{
    const int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (v >= M) return;
    double len, gain;
    int32_t move;
    bme::eval_node(T, ld, bme_view(itab, ldi, t0, top), (int32_t)v, &len, &gain, &move);
    out[v] = len;
    out[ldi + v] = gain;
    omove[v] = move;
}

// the device engine of bme::search: uploads the derived tree, builds the table, brings lengths, gains and moves back
struct DeviceEngine {
    dpr_ctx* c;
    BmeBuffers& B;
    std::vector<int32_t> h_itab;
    hipEvent_t ev[3];
    bool filled = false;
    const double* src = nullptr;
    int64_t sld = 0;
    const int32_t* pos = nullptr;

    int launch_check()
    {
        ++B.launches;
        DPR_HIP(hipGetLastError());
        return DPR_OK;
    }
    int operator()(const bme::Tree& t, bme::Eval& e)
    {
        const int64_t n = t.n, M = t.M, ld = B.ld, ldi = B.ldi;
        const size_t m = (size_t)M;
        const std::vector<int32_t>* arrays[7] = { &t.kid0, &t.kid1, &t.par, &t.sib, &t.height, &t.tin, &t.tout };
        for (int k = 0; k < 7; ++k) std::copy(arrays[k]->begin(), arrays[k]->begin() + (ptrdiff_t)m, h_itab.begin() + (ptrdiff_t)(k * ldi));
        std::copy(t.rows.begin(), t.rows.end(), h_itab.begin() + (ptrdiff_t)(7 * ldi));
        std::copy(t.pos.begin(), t.pos.end(), h_itab.begin() + (ptrdiff_t)(8 * ldi));
        hipStream_t s = c->stream;
        DPR_HIP(hipMemcpyAsync(B.itab, h_itab.data(), sizeof(int32_t) * (size_t)(kItabArrays * ldi), hipMemcpyHostToDevice, s));
        DPR_HIP(hipEventRecord(ev[0], s));
        if (!filled) {
            const int64_t cb = (n + kThreads - 1) / kThreads;
            hipLaunchKernelGGL(bme_fill_kernel, dim3((unsigned)(n * cb)), dim3(kThreads), 0, s, (double*)B.T, ld, n, src, sld, pos, cb);
            if (int rc = launch_check()) return rc;
            filled = true;
        }
        for (int32_t h = 1; h <= t.max_height; ++h) {
            const int64_t r0 = n + t.level[(size_t)h], count = t.level[(size_t)h + 1] - t.level[(size_t)h];
            if (count <= 0) continue;
            const int64_t rb = (count + kTileRows - 1) / kTileRows, cb1 = (r0 + kTileCols - 1) / kTileCols, cb2 = (count + kTileCols - 1) / kTileCols;
            hipLaunchKernelGGL(bme_s_kernel<false>, dim3((unsigned)(rb * cb1)), dim3(kThreads), 0, s, (double*)B.T, ld, n, (const int32_t*)B.itab, ldi, r0,
                               count, cb1);
            if (int rc = launch_check()) return rc;
            if (count < 2) continue;
            hipLaunchKernelGGL(bme_s_kernel<true>, dim3((unsigned)(rb * cb2)), dim3(kThreads), 0, s, (double*)B.T, ld, n, (const int32_t*)B.itab, ldi, r0,
                               count, cb2);
            if (int rc = launch_check()) return rc;
        }
        const int64_t cb = (M + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(bme_w_kernel, dim3((unsigned)cb), dim3(kThreads), 0, s, (double*)B.T, ld, M, (const int32_t*)B.itab, ldi, t.t0, t.top);
        if (int rc = launch_check()) return rc;
        DPR_HIP(hipEventRecord(ev[1], s));
        hipLaunchKernelGGL(bme_len_kernel, dim3((unsigned)cb), dim3(kThreads), 0, s, (const double*)B.T, ld, M, (const int32_t*)B.itab, ldi, t.t0, t.top,
                           (double*)B.out, (int32_t*)B.omove);
        if (int rc = launch_check()) return rc;
        DPR_HIP(hipMemcpyAsync(e.len.data(), B.out, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        DPR_HIP(hipMemcpyAsync(e.gain.data(), B.out + ldi, sizeof(double) * m, hipMemcpyDeviceToHost, s));
        DPR_HIP(hipMemcpyAsync(e.move.data(), B.omove, sizeof(int32_t) * m, hipMemcpyDeviceToHost, s));
        DPR_HIP(hipEventRecord(ev[2], s));
        DPR_HIP(hipStreamSynchronize(s));
        float ms = 0;
        DPR_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        B.table_ms += ms;
        DPR_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
        B.select_ms += ms;
        ++B.evaluations;
        e.sum(M, t.t0);
        return DPR_OK;
    }
};

// buffers for n tips (kept when they already hold as many); a table beyond the device's free memory is refused before any allocation
int bme_reserve(BmeBuffers& B, int64_t n)
{
    if (B.cap_n >= n && B.T) return DPR_OK;
    const int64_t M = 2 * n - 2, ld = (M + 31) / 32 * 32, ldi = ld;
    const size_t need = (size_t)M * (size_t)ld * sizeof(double);
    B.T.reset(); B.itab.reset(); B.out.reset(); B.omove.reset();
    B.cap_n = 0;
    size_t free_b = 0, total_b = 0;
    DPR_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need + (size_t)(64 << 20) > free_b) {
        set_error("dpr_bme_nni: the table of subtree averages over " + std::to_string(M) + " nodes needs " + std::to_string(need) +
                  " bytes, the device has " + std::to_string(free_b) + " free");
        return DPR_ERR_ARG;
    }
    DPR_HIP(B.T.alloc((size_t)M * (size_t)ld));
    DPR_HIP(B.itab.alloc((size_t)(kItabArrays * ldi)));
    DPR_HIP(B.out.alloc((size_t)(2 * ldi)));
    DPR_HIP(B.omove.alloc((size_t)ldi));
    B.allocations += 4;
    B.cap_n = n; B.ld = ld; B.ldi = ldi;
    return DPR_OK;
}

}  // namespace

}  // namespace dpr

using namespace dpr;

extern "C" {

int dpr_bme_nni(dpr_ctx* c, int64_t n, const int32_t* merge_x, const int32_t* merge_y, int max_rounds, int32_t* kids, int32_t* top, double* len,
                double* L_rounds, int64_t* stats4)
{
    if (!c || n < 3 || n >= ((int64_t)1 << 24) || !merge_x || !merge_y || max_rounds < 0 || !kids || !top || !len || !stats4) {
        set_error("dpr_bme_nni: bad argument (n >= 3, max_rounds >= 0, no null output but L_rounds)");
        return DPR_ERR_ARG;
    }
    if (c->world > 1 || c->vworld > 0) {
        set_error("dpr_bme_nni: one rank only (no virtual ranks, no several ranks)");
        return DPR_ERR_ARG;
    }
    if (!c->have_matrix) { set_error("dpr_bme_nni: call dpr_dist_matrix first"); return DPR_ERR_STATE; }
    NjBuffers& b0 = c->nj[0];
    const int kind = c->plan.kind;
    if ((kind != DPR_NJ_PLAN_SINGLE_STREAM && kind != DPR_NJ_PLAN_SINGLE_PRUNED && kind != DPR_NJ_PLAN_BIONJ) || b0.pr.sh_world > 1) {
        set_error("dpr_bme_nni: the context's matrix is shared out (virtual shards); one rank on its own whole copy only");
        return DPR_ERR_ARG;
    }
    if (b0.N != n) { set_error("dpr_bme_nni: n differs from the context's matrix (" + std::to_string(b0.N) + " tips)"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    NjState st;
    if (int rc = fetch_state(c, &st)) return rc;
    if (st.it != 0 || st.n != n) {
        set_error("dpr_bme_nni: the matrix is not fresh (" + std::to_string((long long)st.it) + " NJ iterations since dpr_dist_matrix); build it again");
        return DPR_ERR_STATE;
    }
    bme::Tree t;
    if (!bme::from_merges(n, merge_x, merge_y, t)) { set_error("dpr_bme_nni: not a merge log (0 <= x < y < n - it)"); return DPR_ERR_ARG; }
    BmeBuffers& B = c->bme;
    if (int rc = bme_reserve(B, n)) return rc;
    B.launches = B.evaluations = 0;
    B.table_ms = B.select_ms = 0;
    ScopedEvent e0, e1, e2;
    DPR_HIP(hipEventCreate(e0.put()));
    DPR_HIP(hipEventCreate(e1.put()));
    DPR_HIP(hipEventCreate(e2.put()));
    DeviceEngine eng{ c, B, std::vector<int32_t>((size_t)(kItabArrays * B.ldi), 0), { e0, e1, e2 } };
    if (b0.pr.in_positions()) { eng.src = b0.pr.D; eng.sld = b0.pr.ld; eng.pos = b0.pr.pos_of_slot; }
    else { eng.src = b0.D; eng.sld = b0.ld; }
    bme::Eval cur;
    const int rc = bme::search(t, max_rounds, eng, cur, L_rounds, stats4);
    if (rc) { (void)hipStreamSynchronize(c->stream); (void)hipGetLastError(); return rc; }
    bme::write_outputs(t, cur, kids, top, len);
    return DPR_OK;
}

int dpr_bme_nni_host(const double* lower_rows, int64_t n, const int32_t* merge_x, const int32_t* merge_y, int max_rounds, int32_t* kids,
                     int32_t* top, double* len, double* L_rounds, int64_t* stats4)
{
    if (bme::nni_host(lower_rows, n, merge_x, merge_y, max_rounds, kids, top, len, L_rounds, stats4)) {
        set_error("dpr_bme_nni_host: bad argument, or not a merge log (n >= 3, max_rounds >= 0, 0 <= x < y < n - it)");
        return DPR_ERR_ARG;
    }
    return DPR_OK;
}

int dpr_bme_eval_host(const double* lower_rows, int64_t n, const int32_t* kids, int32_t top, double* len, double* gain, int32_t* move, double* L)
{
    if (bme::eval_host(lower_rows, n, kids, top, len, gain, move, L)) {
        set_error("dpr_bme_eval_host: bad argument, or not a binary tree hung from tip n - 1");
        return DPR_ERR_ARG;
    }
    return DPR_OK;
}

int dpr_get_bme_timing(dpr_ctx* c, double* table_ms, double* select_ms)
{
    if (!c) { set_error("dpr_get_bme_timing: null ctx"); return DPR_ERR_ARG; }
    if (table_ms) *table_ms = c->bme.table_ms;
    if (select_ms) *select_ms = c->bme.select_ms;
    return DPR_OK;
}

int dpr_get_bme_stats(dpr_ctx* c, int64_t* out4)
{
    if (!c || !out4) { set_error("dpr_get_bme_stats: bad argument"); return DPR_ERR_ARG; }
    out4[0] = c->bme.T ? (int64_t)((2 * c->bme.cap_n - 2) * c->bme.ld * (int64_t)sizeof(double)) : 0;
    out4[1] = c->bme.allocations;
    out4[2] = c->bme.launches;
    out4[3] = c->bme.evaluations;
    return DPR_OK;
}

}  // extern "C"
