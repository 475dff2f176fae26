// Fit of a tree to the context's distance matrix on the device: one row pass and one column pass over the lower triangle of the FRESH
// matrix, the path length of every pair from a lowest-common-ancestor lookup.  Contract: include/dipper_hip.h above dpr_tree_fit.
// fit_host.hpp holds what the host and the device share -- the checks of the tree, the depths, the terms of a pair, the combination of
// the parts, the derived figures -- and the restatement behind dpr_tree_fit_host; here are the kernels and the entry points.
//
// Lookup.  The host numbers the tips in depth-first order (rank) and the internal nodes ascending by level (order index), and writes
// gap[r] = order index of lca(tip of rank r, tip of rank r + 1).  lca of the tips of ranks a < b is the shallowest node among
// gap[a .. b): every gap of the range lies in the clade of the lca, and the one descent that leaves tip a's child subtree for tip b's
// is from the lca itself.  A sparse table of range minima over gap answers with two loads, a third gives the node's depth:
//   k = floor(log2(b - a));  o = min(tab[k][a], tab[k][b - 2^k]);  depth = dnode[o].
// The table is 4 (n - 1) (floor(log2(n - 1)) + 1) bytes -- 1.8 MB at 30 000 tips, 6.8 MB at 100 000 -- and is the same for a
// caterpillar as for a balanced tree: nothing is staged per row, no capacity to fall off.
// Row pass      one workgroup of 256 per row i (rows dealt round robin to a fixed grid): thread t takes j = t, t + 256, ... < i, which
//               is the contract's accumulator j mod 256 in ascending order; seven halving trees through LDS; counts and the row's
//               largest |e| through the waves.  A row is read coalesced.
// Column pass   one workgroup of 1 024 per 64 columns: wave w takes the rows i = w mod 16, lane l column j0 + l -- the contract's
//               accumulator i mod 16, i ascending; a wave reads 64 contiguous columns of a row (512 bytes); a halving tree over the 16
//               waves through LDS.
// Both passes write per-taxon parts only; the host adds them up in a fixed order (fit::finish).  No atomics on doubles.
#include "ctx_internal.hpp"

#include "fit_host.hpp"

namespace dpr {

// nj.hip: the yardstick of dpr_ctx_set_fit_compare (reads whole rows of the same matrix once)
__global__ void nj_row_sums_kernel(const double* __restrict__ D, int64_t ld, int64_t N, int64_t rows_local, int rank, int world,
                                   double* __restrict__ U, int local_index);

namespace {

constexpr int kColThreads = 1024;      // column pass: fit::kColAcc waves
constexpr int kColWidth = 64;          // columns of a workgroup of the column pass: one per lane
constexpr int kRowGrid = 4096;         // row pass: workgroups at most
static_assert(kThreads == fit::kRowAcc && kColThreads == 64 * fit::kColAcc, "the accumulators of the contract are threads / waves");

struct FitView {
    const double* src;       // the context's matrix, row stride sld
    int64_t sld;
    const int32_t* pos;      // position of every slot when the matrix lives in position space, else null
    const int32_t* rank;
    const double* dtip;
    const double* dnode;
    const int32_t* tab;      // [levels][g]
    int64_t g, n;            // g = n - 1
};

// depth of lca of two DIFFERENT tips by their ranks; every index lies in [0, g - 2^k]
__device__ inline double lca_depth(const FitView& v, int32_t ra, int32_t rb)
{
    const int32_t lo = ra < rb ? ra : rb, hi = ra < rb ? rb : ra;
    const int k = 31 - __clz(hi - lo);
    const int32_t* row = v.tab + (int64_t)k * v.g;
    const int32_t a = row[lo], b = row[hi - (1 << k)];
    return v.dnode[a < b ? a : b];
}

// matrix entry of the pair {i, j}, i > j, read at (max, min) (bme_fill_kernel's layout logic: a change of the fresh matrix's layouts
// reaches both)
__device__ inline double entry(const FitView& v, int64_t i, int64_t j)
{
    int64_t hi = i, lo = j;
    if (v.pos) { hi = v.pos[hi]; lo = v.pos[lo]; }
    return v.src[hi * v.sld + lo];
}

// Reads the matrix and the tree's tables.  Writes, thread 0 per row i: dpart[q][i] (q < 7 the row parts, 7 the largest |e|) and
// ipart[0 .. 3][i] (counted, counted with D > 0, skipped, j of the largest |e|).  Strides n.
__global__ __launch_bounds__(kThreads) void fit_row_kernel(FitView v, double* __restrict__ dpart, int32_t* __restrict__ ipart)
{
    __shared__ double s[fit::kRowSums][kThreads];
    __shared__ int32_t s_c[3][kThreads / 64], s_j[kThreads / 64];
    __shared__ double s_m[kThreads / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t n = v.n;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        const int32_t ri = v.rank[i];
        const double di = v.dtip[i];
        double a[fit::kRowSums] = { 0, 0, 0, 0, 0, 0, 0 };
        int32_t c = 0, cw = 0, sk = 0, mj = -1;
        double mx = -1.0;
        for (int64_t j = t; j < i; j += kThreads) {
            const double P = fit::patristic(di, v.dtip[j], lca_depth(v, ri, v.rank[j]));
            const fit::Term x = fit::term_of(entry(v, i, j), P);
            if (!x.counted) { ++sk; continue; }
            a[0] = a[0] + x.D; a[1] = a[1] + x.P; a[2] = a[2] + x.DD; a[3] = a[3] + x.PP; a[4] = a[4] + x.DP; a[5] = a[5] + x.ee;
            if (x.weighted) { a[6] = a[6] + x.w; ++cw; }
            ++c;
            if (x.abs_e > mx) { mx = x.abs_e; mj = (int32_t)j; }
        }
#pragma unroll
        for (int q = 0; q < fit::kRowSums; ++q) s[q][t] = a[q];
        for (int off = 32; off > 0; off >>= 1) {
            c += __shfl_down(c, off, 64); cw += __shfl_down(cw, off, 64); sk += __shfl_down(sk, off, 64);
            const double om = __shfl_down(mx, off, 64);
            const int32_t oj = __shfl_down(mj, off, 64);
            if (om > mx || (om == mx && oj < mj)) { mx = om; mj = oj; }
        }
        if (lane == 0) { s_c[0][wave] = c; s_c[1][wave] = cw; s_c[2][wave] = sk; s_m[wave] = mx; s_j[wave] = mj; }
        __syncthreads();
        for (int st = kThreads / 2; st > 0; st >>= 1) {
            if (t < st) {
#pragma unroll
                for (int q = 0; q < fit::kRowSums; ++q) s[q][t] = s[q][t] + s[q][t + st];
            }
            __syncthreads();
        }
        if (t == 0) {
            for (int w = 1; w < kThreads / 64; ++w) {
                c += s_c[0][w]; cw += s_c[1][w]; sk += s_c[2][w];
                if (s_m[w] > mx || (s_m[w] == mx && s_j[w] < mj)) { mx = s_m[w]; mj = s_j[w]; }
            }
            for (int q = 0; q < fit::kRowSums; ++q) dpart[(int64_t)q * n + i] = s[q][0];
            dpart[(int64_t)fit::kRowSums * n + i] = mx;
            ipart[i] = c; ipart[n + i] = cw; ipart[2 * n + i] = sk; ipart[3 * n + i] = mj;
        }
        __syncthreads();      // the LDS entries of this row have been read
    }
}

// Reads the matrix and the tree's tables.  Writes, wave 0: col_ss[j], col_cnt[j] of the workgroup's 64 columns.
__global__ __launch_bounds__(kColThreads) void fit_col_kernel(FitView v, double* __restrict__ col_ss, int32_t* __restrict__ col_cnt)
{
    __shared__ double s[fit::kColAcc][kColWidth];
    __shared__ int32_t s_c[fit::kColAcc][kColWidth];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n = v.n, j0 = (int64_t)blockIdx.x * kColWidth, j = j0 + lane;
    double acc = 0.0;
    int32_t c = 0;
    if (j < n) {
        const int32_t rj = v.rank[j];
        const double dj = v.dtip[j];
        // the first row of this wave's class at or beyond j0 + 1; a lane takes the rows beyond its own column
        int64_t i = (j0 + 1) - (j0 + 1) % fit::kColAcc + wave;
        if (i < j0 + 1) i += fit::kColAcc;
        for (; i < n; i += fit::kColAcc) {
            if (i <= j) continue;
            const double P = fit::patristic(v.dtip[i], dj, lca_depth(v, v.rank[i], rj));
            const fit::Term x = fit::term_of(entry(v, i, j), P);
            if (!x.counted) continue;
            acc = acc + x.ee;
            ++c;
        }
    }
    s[wave][lane] = acc;
    s_c[wave][lane] = c;
    __syncthreads();
    for (int st = fit::kColAcc / 2; st > 0; st >>= 1) {
        if (wave < st) { s[wave][lane] = s[wave][lane] + s[wave + st][lane]; s_c[wave][lane] += s_c[wave + st][lane]; }
        __syncthreads();
    }
    if (wave == 0 && j < n) { col_ss[j] = s[0][lane]; col_cnt[j] = s_c[0][lane]; }
}

// out[r][j] = P of the tips row0 + r and j; grid (column blocks, rows)
__global__ __launch_bounds__(kThreads) void fit_patristic_kernel(FitView v, int64_t row0, double* __restrict__ out)
{
    const int64_t i = row0 + blockIdx.y, j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= v.n || j >= v.n) return;
    const double di = v.dtip[i];
    const double da = i == j ? di : lca_depth(v, v.rank[i], v.rank[j]);
    out[(int64_t)blockIdx.y * v.n + j] = fit::patristic(di, v.dtip[j], da);
}

int table_levels(int64_t n)
{
    int levels = 1;
    while (((int64_t)2 << (levels - 1)) <= n - 1) ++levels;
    return levels;
}

// buffers for n tips (kept when they already hold as many)
int fit_reserve(FitBuffers& B, int64_t n)
{
    if (B.cap_n >= n && B.rank) return DPR_OK;
    B.rank.reset(); B.dtip.reset(); B.dnode.reset(); B.tab.reset(); B.dpart.reset(); B.ipart.reset();
    B.cap_n = 0;
    const size_t cnt = (size_t)n;
    const int levels = table_levels(n);
    DPR_HIP(B.rank.alloc(cnt));
    DPR_HIP(B.dtip.alloc(cnt));
    DPR_HIP(B.dnode.alloc(cnt));
    DPR_HIP(B.tab.alloc(cnt * (size_t)levels));
    DPR_HIP(B.dpart.alloc(cnt * 10));
    DPR_HIP(B.ipart.alloc(cnt * 5));
    B.allocations += 6;
    B.cap_n = n; B.cap_levels = levels;
    return DPR_OK;
}

// the tree's tables to the device (the copies are from pageable memory: done when the calls return)
int fit_upload(FitBuffers& B, const fit::Topo& t, hipStream_t s)
{
    const size_t n = (size_t)t.n;
    DPR_HIP(hipMemcpyAsync(B.rank, t.rank.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, s));
    DPR_HIP(hipMemcpyAsync(B.dtip, t.depth.data(), sizeof(double) * n, hipMemcpyHostToDevice, s));
    DPR_HIP(hipMemcpyAsync(B.dnode, t.dnode.data(), sizeof(double) * t.dnode.size(), hipMemcpyHostToDevice, s));
    DPR_HIP(hipMemcpyAsync(B.tab, t.tab.data(), sizeof(int32_t) * t.tab.size(), hipMemcpyHostToDevice, s));
    return DPR_OK;
}

FitView view_of(const FitBuffers& B, const fit::Topo& t)
{
    return FitView{ nullptr, 0, nullptr, B.rank, B.dtip, B.dnode, B.tab, t.n - 1, t.n };
}

const char* const kTreeRule = ": not a tree as arrays (n + 1 <= m <= 2n - 1 nodes, tips 0 .. n-1 without children, one root with parent -1, every "
                              "other parent an internal node, internal nodes with two children or more, every node reached from the root)";

}  // namespace

}  // namespace dpr

using namespace dpr;

extern "C" {

int dpr_tree_fit(dpr_ctx* c, int64_t n, int64_t m, const int32_t* parent, const double* len, double* sums, double* taxon_ss, int64_t* taxon_pairs,
                 int32_t* worst)
{
    const std::string who = "dpr_tree_fit";
    if (!c || n < 2 || n >= ((int64_t)1 << 24) || !parent || !len || !sums || !taxon_ss || !taxon_pairs || !worst) {
        set_error(who + ": bad argument (2 <= n < 2^24, no null pointer)");
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
    fit::Topo t;
    if (fit::prepare(n, m, parent, len, t, true)) { set_error(who + kTreeRule); return DPR_ERR_ARG; }
    FitBuffers& B = c->fit;
    if (int rc = fit_reserve(B, n)) return rc;
    B.launches = 0; B.levels = t.levels; B.row_ms = 0; B.col_ms = 0; B.rowsum_ms = 0;
    hipStream_t s = c->stream;
    if (int rc = fit_upload(B, t, s)) return rc;
    FitView v = view_of(B, t);
    if (b0.pr.in_positions()) { v.src = b0.pr.D; v.sld = b0.pr.ld; v.pos = b0.pr.pos_of_slot; }
    else { v.src = b0.D; v.sld = b0.ld; }
    double* dpart = B.dpart;
    int32_t* ipart = B.ipart;
    ScopedEvent e0, er, e1, e2;
    DPR_HIP(hipEventCreate(e0.put()));
    DPR_HIP(hipEventCreate(er.put()));
    DPR_HIP(hipEventCreate(e1.put()));
    DPR_HIP(hipEventCreate(e2.put()));
    DPR_HIP(hipEventRecord(e0, s));
    hipLaunchKernelGGL(fit_row_kernel, dim3((unsigned)(n < kRowGrid ? n : kRowGrid)), dim3(kThreads), 0, s, v, dpart, ipart);
    DPR_HIP(hipEventRecord(er, s));
    hipLaunchKernelGGL(fit_col_kernel, dim3((unsigned)((n + kColWidth - 1) / kColWidth)), dim3(kColThreads), 0, s, v, dpart + 8 * n, ipart + 4 * n);
    B.launches += 2;
    DPR_HIP(hipGetLastError());
    DPR_HIP(hipEventRecord(e1, s));
    if (B.compare) {
        hipLaunchKernelGGL(nj_row_sums_kernel, dim3((unsigned)(n < kRowGrid ? n : kRowGrid)), dim3(kThreads), 0, s, v.src, v.sld, n, n, 0, 1, dpart + 9 * n, 0);
        ++B.launches;
        DPR_HIP(hipGetLastError());
        DPR_HIP(hipEventRecord(e2, s));
    }
    const size_t N = (size_t)n;
    fit::Parts p;
    p.size(N);
    DPR_HIP(hipMemcpyAsync(p.row.data(), dpart, sizeof(double) * N * fit::kRowSums, hipMemcpyDeviceToHost, s));
    DPR_HIP(hipMemcpyAsync(p.max_e.data(), dpart + 7 * n, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    DPR_HIP(hipMemcpyAsync(p.col_ss.data(), dpart + 8 * n, sizeof(double) * N, hipMemcpyDeviceToHost, s));
    DPR_HIP(hipMemcpyAsync(p.cnt.data(), ipart, sizeof(int32_t) * N * 3, hipMemcpyDeviceToHost, s));
    DPR_HIP(hipMemcpyAsync(p.arg_j.data(), ipart + 3 * n, sizeof(int32_t) * N, hipMemcpyDeviceToHost, s));
    DPR_HIP(hipMemcpyAsync(p.col_cnt.data(), ipart + 4 * n, sizeof(int32_t) * N, hipMemcpyDeviceToHost, s));
    DPR_HIP(hipStreamSynchronize(s));
    float ms = 0;
    DPR_HIP(hipEventElapsedTime(&ms, e0, er));
    B.row_ms = ms;
    DPR_HIP(hipEventElapsedTime(&ms, er, e1));
    B.col_ms = ms;
    if (B.compare) {
        DPR_HIP(hipEventElapsedTime(&ms, e1, e2));
        B.rowsum_ms = ms;
    }
    fit::finish(n, p, sums, taxon_ss, taxon_pairs, worst);
    return DPR_OK;
}

int dpr_tree_fit_host(const double* lower_rows, int64_t n, int64_t m, const int32_t* parent, const double* len, double* sums, double* taxon_ss,
                      int64_t* taxon_pairs, int32_t* worst)
{
    if (fit::fit_host(lower_rows, n, m, parent, len, sums, taxon_ss, taxon_pairs, worst)) {
        set_error(std::string("dpr_tree_fit_host: a null pointer, or") + (kTreeRule + 1));
        return DPR_ERR_ARG;
    }
    return DPR_OK;
}

int dpr_tree_fit_derive(double* sums)
{
    if (!sums) { set_error("dpr_tree_fit_derive: null sums"); return DPR_ERR_ARG; }
    fit::derive(sums);
    return DPR_OK;
}

int dpr_tree_patristic_rows(dpr_ctx* c, int64_t n, int64_t m, const int32_t* parent, const double* len, int64_t row0, int64_t nrows, double* out)
{
    const std::string who = "dpr_tree_patristic_rows";
    if (!c || n < 2 || n >= ((int64_t)1 << 24) || !parent || !len || !out || row0 < 0 || nrows < 1 || row0 + nrows > n || nrows > 65535) {
        set_error(who + ": bad argument (2 <= n < 2^24, 0 <= row0, 1 <= nrows <= 65535, row0 + nrows <= n, no null pointer)");
        return DPR_ERR_ARG;
    }
    fit::Topo t;
    if (fit::prepare(n, m, parent, len, t, true)) { set_error(who + kTreeRule); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    FitBuffers& B = c->fit;
    if (int rc = fit_reserve(B, n)) return rc;
    hipStream_t s = c->stream;
    if (int rc = fit_upload(B, t, s)) return rc;
    DevBuf<double> rows;
    DPR_HIP(rows.alloc((size_t)nrows * (size_t)n));
    const FitView v = view_of(B, t);
    hipLaunchKernelGGL(fit_patristic_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads), (unsigned)nrows), dim3(kThreads), 0, s, v, row0, (double*)rows);
    DPR_HIP(hipGetLastError());
    DPR_HIP(hipMemcpyAsync(out, rows, sizeof(double) * (size_t)nrows * (size_t)n, hipMemcpyDeviceToHost, s));
    DPR_HIP(hipStreamSynchronize(s));
    return DPR_OK;
}

int dpr_tree_from_nj(int64_t n, const int32_t* merge_x, const int32_t* merge_y, const double* bx, const double* by, double last, int32_t* parent,
                     double* len, int64_t* m)
{
    if (fit::from_nj(n, merge_x, merge_y, bx, by, last, parent, len, m)) {
        set_error("dpr_tree_from_nj: bad argument, or not a merge log (n >= 2, 0 <= x, y < n - it, x != y)");
        return DPR_ERR_ARG;
    }
    return DPR_OK;
}

int dpr_tree_from_kids(int64_t n, const int32_t* kids, int32_t top, const double* len_in, int32_t* parent, double* len, int64_t* m)
{
    if (fit::from_kids(n, kids, top, len_in, parent, len, m)) {
        set_error("dpr_tree_from_kids: bad argument, or not a binary tree over nodes 0 .. 2n-3 hung from tip n - 1");
        return DPR_ERR_ARG;
    }
    return DPR_OK;
}

int dpr_tree_from_upgma(int64_t n, const int32_t* merge_x, const int32_t* merge_y, const double* height, int32_t* parent, double* len, int64_t* m)
{
    if (fit::from_upgma(n, merge_x, merge_y, height, parent, len, m)) {
        set_error("dpr_tree_from_upgma: bad argument, or not a merge log (n >= 2, 0 <= x, y < n - it, x != y)");
        return DPR_ERR_ARG;
    }
    return DPR_OK;
}

int dpr_get_fit_stats(dpr_ctx* c, int64_t* out4)
{
    if (!c || !out4) { set_error("dpr_get_fit_stats: bad argument"); return DPR_ERR_ARG; }
    const FitBuffers& B = c->fit;
    out4[0] = B.rank ? B.cap_n * (int64_t)(4 + 8 + 8 + 4 * B.cap_levels + 10 * 8 + 5 * 4) : 0;
    out4[1] = B.allocations;
    out4[2] = B.launches;
    out4[3] = B.levels;
    return DPR_OK;
}

int dpr_get_fit_timing(dpr_ctx* c, double* row_ms, double* col_ms, double* rowsum_ms)
{
    if (!c) { set_error("dpr_get_fit_timing: null ctx"); return DPR_ERR_ARG; }
    if (row_ms) *row_ms = c->fit.row_ms;
    if (col_ms) *col_ms = c->fit.col_ms;
    if (rowsum_ms) *rowsum_ms = c->fit.rowsum_ms;
    return DPR_OK;
}

int dpr_ctx_set_fit_compare(dpr_ctx* c, int on)
{
    if (!c) { set_error("dpr_ctx_set_fit_compare: null ctx"); return DPR_ERR_ARG; }
    c->fit.compare = on ? 1 : 0;
    return DPR_OK;
}

}  // extern "C"
