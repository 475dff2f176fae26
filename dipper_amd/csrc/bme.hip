// Balanced minimum evolution (Desper & Gascuel 2002; no reference counterpart: the reference stops at the NJ tree): NNI search
// from the tree of a merge log, and the balanced branch lengths of the tree it ends on.  Contract: include/dipper_hip.h above
// dpr_bme_nni.  bme_host.hpp holds what the host and the device share -- the tree, the selection, the search loop and the per-node
// arithmetic -- and the host engine of dpr_bme_nni_host; here are the device engine and the entry points.  The SPR search of
// dpr_bme_spr evaluates a tree the same way and then scans it: its kernels and engine follow the NNI engine below.
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
int bme_reserve(BmeBuffers& B, int64_t n, const char* who = "dpr_bme_nni")
{
    if (B.cap_n >= n && B.T) return DPR_OK;
    const int64_t M = 2 * n - 2, ld = (M + 31) / 32 * 32, ldi = ld;
    const size_t need = (size_t)M * (size_t)ld * sizeof(double);
    B.T.reset(); B.itab.reset(); B.out.reset(); B.omove.reset();
    B.cap_n = 0;
    size_t free_b = 0, total_b = 0;
    DPR_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need + (size_t)(64 << 20) > free_b) {
        set_error(std::string(who) + ": the table of subtree averages over " + std::to_string(M) + " nodes needs " + std::to_string(need) +
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

// ---- SPR scan (contract: include/dipper_hip.h above dpr_bme_spr; the arithmetic is bme::spr_step) ---------------------------------
// After the table of an evaluation: W is mirrored into the elements above the diagonal of ancestry (one thread per node climbs to
// the top), then one thread per (directed subtree X, side of q the path leaves through) walks the rest of the tree depth first.
// A path node costs one 16-byte record and seven table elements -- the rows of X and A gathered at the places of the two
// continuations, three elements between the continuations and the way back -- and gives two candidates; U and V ride along the
// path.  Where both continuations are internal the larger one is stacked, so a thread's stack stays below log2 M entries; the
// stacks live in one buffer of the context, one column per resident thread.  No lane waits for another inside a traversal: the
// loops are per lane and bounded by M.  The best (gain, w, k) of every (X, side) goes to a partial array, a second kernel takes
// the better side per X, and only those 3 x 2M values go back to the host.  Three of the seven elements do not depend on X: a
// kernel before the scan gathers them per node (bme_spr_trio_kernel), which leaves four table elements a path node.
constexpr int64_t kSprWorkers = 131072;      // resident scan threads: 2 waves on every SIMD of 256 compute units

struct SprDevStack {
    double* d;
    int32_t* i;
    int64_t W, me;
    int sp;
    __device__ void push(int32_t p, int32_t from, int32_t k, double U, double V, double h)
    {
        if (sp >= bme::kSprStack) return;
        const int64_t at = (int64_t)sp * 3 * W + me;
        d[at] = U; d[at + W] = V; d[at + 2 * W] = h;
        i[at] = p; i[at + W] = from; i[at + 2 * W] = k;
        ++sp;
    }
    __device__ bool pop(bme::SprState& s)
    {
        if (sp == 0) return false;
        const int64_t at = (int64_t)(--sp) * 3 * W + me;
        s.U = d[at]; s.V = d[at + W]; s.h = d[at + 2 * W];
        s.p = i[at]; s.from = i[at + W]; s.k = i[at + 2 * W];
        return true;
    }
};

__global__ __launch_bounds__(kThreads) void bme_spr_mirror_kernel(double* __restrict__ T, int64_t ld, int64_t M, const int32_t* __restrict__ itab,
                                                                  int64_t ldi, int32_t t0, int32_t top)
{
    const int64_t u = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (u >= M) return;
    bme::spr_mirror_w(T, ld, M, bme_view(itab, ldi, t0, top), (int32_t)u);
}

// The three averages between the three subtrees at an internal node (bme::SprTree::trio): what a path node contributes to a gain
// whatever X is, gathered once per node instead of once per (X, node) -- the table is far larger than any cache, these 24 bytes
// a node are not.  One thread per internal place.
__global__ __launch_bounds__(kThreads) void bme_spr_trio_kernel(const double* __restrict__ T, int64_t ld, int32_t n, int32_t M,
                                                                const int32_t* __restrict__ tab, int32_t t0, int32_t top, double* __restrict__ trio)
{
    const int64_t p = (int64_t)n + (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= M) return;
    const bme::SprRec r = reinterpret_cast<const bme::SprRec*>(tab)[p];
    const int64_t up = p == top ? t0 : p;
    trio[3 * p] = T[(int64_t)r.k0 * ld + r.k1];
    trio[3 * p + 1] = T[(int64_t)r.k0 * ld + up];
    trio[3 * p + 2] = T[(int64_t)r.k1 * ld + up];
}

// tab: 4 ints of record per place, then (at 4 ldi) the node id of every place; t0 and top are places here.  W = threads of the grid.
__global__ __launch_bounds__(kThreads) void bme_spr_scan_kernel(const double* __restrict__ T, int64_t ld, int32_t n, int32_t M,
                                                                const int32_t* __restrict__ tab, int64_t ldi, int32_t t0, int32_t top,
                                                                const double* __restrict__ trio, double* __restrict__ dstack, int32_t* __restrict__ istack, int64_t W,
                                                                double* __restrict__ pg, int32_t* __restrict__ pw, int32_t* __restrict__ pk)
{
    const int64_t me = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const bme::SprTree t{ T, ld, reinterpret_cast<const bme::SprRec*>(tab), tab + 4 * ldi, trio, n, M, t0, top };
    SprDevStack st{ dstack, istack, W, me, 0 };
    const int64_t items = 4 * (int64_t)M;
    for (int64_t item = me; item < items; item += W) {
        const int32_t dp = (int32_t)(item >> 1);
        bme::SprBest b;
        bme::SprState s;
        bool live = bme::spr_begin(t, dp, (int)(item & 1), s);
        for (int64_t step = 0; live && step < M; ++step) live = bme::spr_step(t, s, b, st);
        st.sp = 0;
        const int64_t d = dp >= M ? (int64_t)M + t.id(dp - M) : (int64_t)t.id(dp);
        const int64_t o = 2 * d + (item & 1);
        pg[o] = b.g; pw[o] = b.w; pk[o] = b.k;
    }
}

__global__ __launch_bounds__(kThreads) void bme_spr_best_kernel(int64_t count, const double* __restrict__ pg, const int32_t* __restrict__ pw,
                                                                const int32_t* __restrict__ pk, double* __restrict__ g, int32_t* __restrict__ w,
                                                                int32_t* __restrict__ k)
{
    const int64_t d = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (d >= count) return;
    bme::SprBest b;
    b.g = pg[2 * d]; b.w = pw[2 * d]; b.k = pk[2 * d];
    if (pk[2 * d + 1] != 0) b.merge(pg[2 * d + 1], pw[2 * d + 1], pk[2 * d + 1]);
    g[d] = b.g; w[d] = b.w; k[d] = b.k;
}

// the SPR buffers beside the table (sized by its stride; the stacks by the resident threads alone)
int spr_reserve(BmeBuffers& B)
{
    if (!B.spr_dstack) {
        DPR_HIP(B.spr_dstack.alloc((size_t)(kSprWorkers * 3 * bme::kSprStack)));
        DPR_HIP(B.spr_istack.alloc((size_t)(kSprWorkers * 3 * bme::kSprStack)));
        B.spr_allocations += 2;
    }
    if (B.spr_ldi >= B.ldi && B.spr_tab) return DPR_OK;
    B.spr_tab.reset(); B.spr_gain.reset(); B.spr_wk.reset();
    B.spr_ldi = 0;
    DPR_HIP(B.spr_tab.alloc((size_t)(5 * B.ldi)));
    DPR_HIP(B.spr_gain.alloc((size_t)(9 * B.ldi)));
    DPR_HIP(B.spr_wk.alloc((size_t)(12 * B.ldi)));
    B.spr_allocations += 3;
    B.spr_ldi = B.ldi;
    return DPR_OK;
}

// the device engine of bme::spr_search: the evaluation of DeviceEngine, then the scan on the table it left
struct SprDeviceEngine {
    DeviceEngine& base;
    std::vector<int32_t> h_tab;
    hipEvent_t ev[2];
    int operator()(const bme::Tree& t, bme::Eval& e, bme::SprEval& se)
    {
        if (int rc = base(t, e)) return rc;
        BmeBuffers& B = base.B;
        const int64_t M = t.M, ld = B.ld, ldi = B.ldi, L = B.spr_ldi;
        hipStream_t s = base.c->stream;
        bme::spr_records(t, true, h_tab.data(), 4 * L);
        DPR_HIP(hipMemcpyAsync(B.spr_tab, h_tab.data(), sizeof(int32_t) * (size_t)(5 * L), hipMemcpyHostToDevice, s));
        DPR_HIP(hipEventRecord(ev[0], s));
        const int64_t cb = (M + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(bme_spr_mirror_kernel, dim3((unsigned)cb), dim3(kThreads), 0, s, (double*)B.T, ld, M, (const int32_t*)B.itab, ldi, t.t0, t.top);
        if (int rc = base.launch_check()) return rc;
        const int64_t blocks = std::min(kSprWorkers, (4 * M + kThreads - 1) / kThreads * kThreads) / kThreads;
        double* pg = B.spr_gain;
        int32_t* pw = B.spr_wk;
        int32_t* pk = pw + 4 * L;
        double* fg = pg + 4 * L;
        double* trio = pg + 6 * L;
        const int32_t t0p = t.pos[(size_t)t.t0], topp = t.pos[(size_t)t.top];
        hipLaunchKernelGGL(bme_spr_trio_kernel, dim3((unsigned)((t.n - 2 + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, (const double*)B.T, ld,
                           (int32_t)t.n, (int32_t)M, (const int32_t*)B.spr_tab, t0p, topp, trio);
        if (int rc = base.launch_check()) return rc;
        int32_t* fw = pw + 8 * L;
        int32_t* fk = pw + 10 * L;
        hipLaunchKernelGGL(bme_spr_scan_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, (const double*)B.T, ld, (int32_t)t.n, (int32_t)M,
                           (const int32_t*)B.spr_tab, L, t0p, topp, (const double*)trio, (double*)B.spr_dstack, (int32_t*)B.spr_istack,
                           blocks * kThreads, pg, pw, pk);
        if (int rc = base.launch_check()) return rc;
        const int64_t db = (2 * M + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(bme_spr_best_kernel, dim3((unsigned)db), dim3(kThreads), 0, s, 2 * M, (const double*)pg, (const int32_t*)pw,
                           (const int32_t*)pk, fg, fw, fk);
        if (int rc = base.launch_check()) return rc;
        DPR_HIP(hipMemcpyAsync(se.gain.data(), fg, sizeof(double) * (size_t)(2 * M), hipMemcpyDeviceToHost, s));
        DPR_HIP(hipMemcpyAsync(se.w.data(), fw, sizeof(int32_t) * (size_t)(2 * M), hipMemcpyDeviceToHost, s));
        DPR_HIP(hipMemcpyAsync(se.k.data(), fk, sizeof(int32_t) * (size_t)(2 * M), hipMemcpyDeviceToHost, s));
        DPR_HIP(hipEventRecord(ev[1], s));
        DPR_HIP(hipStreamSynchronize(s));
        float ms = 0;
        DPR_HIP(hipEventElapsedTime(&ms, ev[0], ev[1]));
        B.spr_scan_ms += ms;
        B.spr_launches += 4;
        return DPR_OK;
    }
};

}  // namespace

}  // namespace dpr

using namespace dpr;

extern "C" {

// dpr_bme_nni (spr = false, 4 stats) and dpr_bme_spr (6 stats): the same preconditions, table and outputs
static int bme_run(dpr_ctx* c, int64_t n, const int32_t* merge_x, const int32_t* merge_y, int max_rounds, int32_t* kids, int32_t* top, double* len,
                   double* L_rounds, int64_t* stats, bool spr)
{
    const std::string who = spr ? "dpr_bme_spr" : "dpr_bme_nni";
    int64_t* stats4 = stats;
    if (!c || n < 3 || n >= ((int64_t)1 << 24) || !merge_x || !merge_y || max_rounds < 0 || !kids || !top || !len || !stats4) {
        set_error(who + ": bad argument (n >= 3, max_rounds >= 0, no null output but L_rounds)");
        return DPR_ERR_ARG;
    }
    if (c->world > 1 || c->vworld > 0) {
        set_error(who + ": one rank only (no virtual ranks, no several ranks)");
        return DPR_ERR_ARG;
    }
    if (!c->have_matrix) { set_error(who + ": call dpr_dist_matrix first"); return DPR_ERR_STATE; }
    NjBuffers& b0 = c->nj[0];
    const int kind = c->plan.kind;
    if ((kind != DPR_NJ_PLAN_SINGLE_STREAM && kind != DPR_NJ_PLAN_SINGLE_PRUNED && kind != DPR_NJ_PLAN_BIONJ) || b0.pr.sh_world > 1) {
        set_error(who + ": the context's matrix is shared out (virtual shards); one rank on its own whole copy only");
        return DPR_ERR_ARG;
    }
    if (b0.N != n) { set_error(who + ": n differs from the context's matrix (" + std::to_string(b0.N) + " tips)"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    NjState st;
    if (int rc = fetch_state(c, &st)) return rc;
    if (st.it != 0 || st.n != n) {
        set_error(who + ": the matrix is not fresh (" + std::to_string((long long)st.it) + " NJ iterations since dpr_dist_matrix); build it again");
        return DPR_ERR_STATE;
    }
    bme::Tree t;
    if (!bme::from_merges(n, merge_x, merge_y, t)) { set_error(who + ": not a merge log (0 <= x < y < n - it)"); return DPR_ERR_ARG; }
    BmeBuffers& B = c->bme;
    if (int rc = bme_reserve(B, n, who.c_str())) return rc;
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
    int rc;
    if (spr) {
        if (int rs = spr_reserve(B)) return rs;
        B.spr_scan_ms = 0;
        B.spr_launches = 0;
        ScopedEvent s0, s1;
        DPR_HIP(hipEventCreate(s0.put()));
        DPR_HIP(hipEventCreate(s1.put()));
        SprDeviceEngine seng{ eng, std::vector<int32_t>((size_t)(5 * B.spr_ldi), 0), { s0, s1 } };
        rc = bme::spr_search(t, max_rounds, seng, cur, L_rounds, stats);
        if (rc < 0 && rc != DPR_ERR_HIP) { set_error(who + ": a selected move did not give a tree (internal)"); rc = DPR_ERR_STATE; }
    } else {
        rc = bme::search(t, max_rounds, eng, cur, L_rounds, stats4);
    }
    if (rc) { (void)hipStreamSynchronize(c->stream); (void)hipGetLastError(); return rc; }
    bme::write_outputs(t, cur, kids, top, len);
    return DPR_OK;
}

int dpr_bme_nni(dpr_ctx* c, int64_t n, const int32_t* merge_x, const int32_t* merge_y, int max_rounds, int32_t* kids, int32_t* top, double* len,
                double* L_rounds, int64_t* stats4)
{
    return bme_run(c, n, merge_x, merge_y, max_rounds, kids, top, len, L_rounds, stats4, false);
}

int dpr_bme_spr(dpr_ctx* c, int64_t n, const int32_t* merge_x, const int32_t* merge_y, int max_rounds, int32_t* kids, int32_t* top, double* len,
                double* L_rounds, int64_t* stats6)
{
    return bme_run(c, n, merge_x, merge_y, max_rounds, kids, top, len, L_rounds, stats6, true);
}

int dpr_bme_spr_host(const double* lower_rows, int64_t n, const int32_t* merge_x, const int32_t* merge_y, int max_rounds, int32_t* kids,
                     int32_t* top, double* len, double* L_rounds, int64_t* stats6)
{
    if (bme::spr_host(lower_rows, n, merge_x, merge_y, max_rounds, kids, top, len, L_rounds, stats6)) {
        set_error("dpr_bme_spr_host: bad argument, or not a merge log (n >= 3, max_rounds >= 0, 0 <= x < y < n - it)");
        return DPR_ERR_ARG;
    }
    return DPR_OK;
}

int dpr_bme_spr_eval_host(const double* lower_rows, int64_t n, const int32_t* kids, int32_t top, double* best_gain, int32_t* best_w, int32_t* best_k,
                          double* L)
{
    if (bme::spr_eval_host(lower_rows, n, kids, top, -1, -1, best_gain, best_w, best_k, L)) {
        set_error("dpr_bme_spr_eval_host: bad argument, or not a binary tree hung from tip n - 1");
        return DPR_ERR_ARG;
    }
    return DPR_OK;
}

int dpr_bme_spr_gain_host(const double* lower_rows, int64_t n, const int32_t* kids, int32_t top, int64_t d, int32_t w, double* gain, int32_t* k)
{
    const int rc = d < 0 ? -1 : bme::spr_eval_host(lower_rows, n, kids, top, d, w, gain, nullptr, k, nullptr);
    if (rc) {
        set_error(rc == -2 ? "dpr_bme_spr_gain_host: w is no target of the directed subtree d"
                           : "dpr_bme_spr_gain_host: bad argument, or not a binary tree hung from tip n - 1");
        return DPR_ERR_ARG;
    }
    return DPR_OK;
}

int dpr_get_bme_spr_timing(dpr_ctx* c, double* scan_ms)
{
    if (!c) { set_error("dpr_get_bme_spr_timing: null ctx"); return DPR_ERR_ARG; }
    if (scan_ms) *scan_ms = c->bme.spr_scan_ms;
    return DPR_OK;
}

int dpr_get_bme_spr_stats(dpr_ctx* c, int64_t* out4)
{
    if (!c || !out4) { set_error("dpr_get_bme_spr_stats: bad argument"); return DPR_ERR_ARG; }
    const BmeBuffers& B = c->bme;
    out4[0] = B.spr_dstack ? (int64_t)(kSprWorkers * 3 * bme::kSprStack * (int64_t)(sizeof(double) + sizeof(int32_t))) : 0;
    out4[1] = B.spr_allocations;
    out4[2] = B.spr_launches;
    out4[3] = kSprWorkers;
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
