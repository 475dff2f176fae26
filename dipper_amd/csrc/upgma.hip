// UPGMA / WPGMA on the device (average-linkage clustering: the rooted, ultrametric distance method; no reference counterpart).
// Contract: include/dipper_hip.h above dpr_upgma_run.  upgma_host.hpp holds what the host and the device share -- the order of
// values and the update arithmetic -- and the naive restatement behind dpr_upgma_host; here are the device loop and the entry points.
//
// The loop works on a square copy D of the context's fresh matrix (both triangles, row stride ld) and keeps, per active row k, its
// nearest neighbour (nkey[k], nn[k]) = the smallest (key(D[k][j]), j) over j != k.  The pair the contract selects is then the
// smallest (nkey[k], min(k, nn[k]), max(k, nn[k])) over the rows: the row of the winning i has all its tied partners above i and
// the smallest of them is j.  One iteration is three launches that take everything from device memory:
//   pick     one workgroup reduces the m cache entries, writes the log entry, the merged sizes and the iteration's state;
//   update   one thread per slot k: the new distances into row x and column x, slot m-1 into y, the caches of the rows that
//            did not merge (compared against the two changed columns, ALWAYS: a weighted mean can round an ulp below both
//            its terms, and renaming m-1 to y can make y the smaller of two tied partners), the list of rows to scan again;
//   rescan   a fixed grid whose workgroups take list entries: one row of m - 1 doubles each, 16-byte loads, (key, j) reduced
//            through the wave and LDS.
// The iteration number goes round three words (it_a -> it_b -> it_c -> it_a), each written by one thread of the launch before
// the one that reads it: nothing a launch reads is written by another thread of the same launch.  Every loop is bounded by m.
// What bounds it: launch latency (three dependent launches) while few rows are listed; the rescans on inputs full of ties (an
// all-equal matrix lists every row every iteration: m^2 / 2 elements read an iteration, right but slow).
#include "ctx_internal.hpp"

#include "upgma_host.hpp"

namespace dpr {

namespace {

constexpr int kPickThreads = 1024;      // pick: one workgroup whatever m is (30 000 entries: 30 per thread)
constexpr int kRescanThreads = 1024;      // rescan: one workgroup per listed row
constexpr int kRescanBlocks = 128;        // rescan: fixed grid
constexpr uint64_t kNoPair = ~(uint64_t)0;

struct UpgmaState {
    int64_t n;                          // tips
    int64_t it_a, it_b, it_c;           // iteration pick / update / rescan works on (rescan: the one whose merge it follows, + 1)
    int32_t x, y;                       // slots merged by the iteration (x < y)
    double sx, sy;                      // their sizes before the merge
    int32_t linkage;
    unsigned int nres;                  // rows listed for the rescan of this iteration
    unsigned long long rescanned;       // rows rescanned since the start of the call (the first fill of the cache not counted)
};

// (key, pair) ascending; pair = i << 32 | j
__device__ inline bool pair_less(uint64_t ka, uint64_t pa, uint64_t kb, uint64_t pb) { return ka < kb || (ka == kb && pa < pb); }

// the smallest (k, p) of the workgroup in thread 0; s_k / s_p: one entry per wave
template <int kBlock>
__device__ inline void block_min(uint64_t& k, uint64_t& p, uint64_t* s_k, uint64_t* s_p)
{
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t ok = __shfl_down((unsigned long long)k, off, 64), op = __shfl_down((unsigned long long)p, off, 64);
        if (pair_less(ok, op, k, p)) { k = ok; p = op; }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { s_k[wave] = k; s_p[wave] = p; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kBlock / 64; ++w)
            if (pair_less(s_k[w], s_p[w], k, p)) { k = s_k[w]; p = s_p[w]; }
}

// D[i][j] = matrix entry of the pair {i, j}, read at (max, min).  src: the context's matrix, row stride sld; pos: position of
// every slot when the matrix lives in position space, else null.  One block: 256 columns of one row.  Reads src, writes D.
// (bme_fill_kernel's layout logic, line for line: a change of the fresh matrix's layouts reaches both.)
__global__ __launch_bounds__(kThreads) void upgma_fill_kernel(double* __restrict__ D, int64_t ld, int64_t n, const double* __restrict__ src,
                                                              int64_t sld, const int32_t* __restrict__ pos, int64_t colblocks)
{
    const int64_t i = blockIdx.x / colblocks, j = (blockIdx.x % colblocks) * kThreads + threadIdx.x;
    if (i >= n || j >= n || i == j) return;      // the diagonal is never used: a row scan loads it and skips it
    int64_t hi = i > j ? i : j, lo = i > j ? j : i;
    if (pos) { hi = pos[hi]; lo = pos[lo]; }
    D[i * ld + j] = src[hi * sld + lo];
}

// Start of a call.  Writes the state, the sizes and the list of the first rescan (every row).  Reads nothing.
__global__ __launch_bounds__(kThreads) void upgma_init_kernel(UpgmaState* __restrict__ st, double* __restrict__ size, int32_t* __restrict__ list,
                                                              int64_t n, int linkage)
{
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (k < n) { size[k] = 1.0; list[k] = (int32_t)k; }
    if (k == 0) {
        st->n = n; st->it_a = 0; st->it_b = 0; st->it_c = 0;
        st->x = 0; st->y = 1; st->sx = 1.0; st->sy = 1.0;
        st->linkage = linkage; st->nres = (unsigned int)n; st->rescanned = 0;
    }
}

// Reads: st->n, st->it_a; nkey, nn of the m = n - it_a active rows; D[y][x], size[x], size[y], size[m-1] (thread 0 only, after
// the reduction).  Writes (thread 0 only): the log entry; st->it_b, x, y, sx, sy, nres = 0; size[x], size[y].  One workgroup.
__global__ __launch_bounds__(kPickThreads) void upgma_pick_kernel(UpgmaState* __restrict__ st, const uint64_t* __restrict__ nkey,
                                                                  const int32_t* __restrict__ nn, const double* __restrict__ D, int64_t ld,
                                                                  double* __restrict__ size, int32_t* __restrict__ merge_x,
                                                                  int32_t* __restrict__ merge_y, double* __restrict__ height)
{
    __shared__ uint64_t s_k[kPickThreads / 64], s_p[kPickThreads / 64];
    const int64_t n = st->n, it = st->it_a, m = n - it;
    if (m < 2) return;
    uint64_t bk = kNoPair, bp = kNoPair;
    for (int64_t k = threadIdx.x; k < m; k += kPickThreads) {
        const int64_t j = nn[k];
        const uint64_t p = k < j ? ((uint64_t)k << 32 | (uint64_t)j) : ((uint64_t)j << 32 | (uint64_t)k);
        const uint64_t q = nkey[k];
        if (pair_less(q, p, bk, bp)) { bk = q; bp = p; }
    }
    block_min<kPickThreads>(bk, bp, s_k, s_p);
    if (threadIdx.x != 0) return;
    int64_t x = (int64_t)(bp >> 32), y = (int64_t)(bp & 0xffffffffu);
    if (!(x < y && y < m)) { x = 0; y = 1; }      // cannot happen with a whole cache; keeps every index inside the matrix
    const int64_t last = m - 1;
    const double d = D[y * ld + x], sx = size[x], sy = size[y];
    merge_x[it] = (int32_t)x;
    merge_y[it] = (int32_t)y;
    height[it] = 0.5 * d;
    size[x] = sx + sy;
    if (y != last) size[y] = size[last];
    st->x = (int32_t)x; st->y = (int32_t)y; st->sx = sx; st->sy = sy;
    st->nres = 0;
    st->it_b = it;
}

__device__ inline void cache_take(uint64_t& ck, int32_t& cj, double v, int32_t j)
{
    const uint64_t q = upgma::key(v);
    if (q < ck || (q == ck && j < cj)) { ck = q; cj = j; }
}

// One thread per slot k < m = n - it_b, last = m - 1, moved = (y != last).
// Reads: st (n, it_b, x, y, sx, sy, linkage); D[x][k], D[y][k], D[last][k], D[k][last]; nkey[k], nn[k] -- thread k alone reads
// what it names, and of these only D[x][k], D[y][k] (after its own reads) and its own cache are written, by itself.
// Writes, k other than x, y, and other than last when a slot moves: D[x][k] = D[k][x] = val; when a slot moves D[y][k] = D[last][k],
// D[k][y] = D[k][last]; nkey[k], nn[k].  k = last when it moves: its val to D[x][y] and D[y][x], which no thread of the launch
// reads (threads x and y read nothing of the matrix) and no other writes -- here the row move and the column writes meet.
// Rows x, y (the moved row) and every row whose nearest neighbour was x or y are appended to list (atomic counter st->nres,
// which the launch does not read otherwise).  Row y is listed even when no slot moves into it (y = last): scanning the vacated
// row once is wasted work in about 2 of m iterations and keeps `two rows an iteration` a floor the counter can be held to.
// Thread x writes st->it_c.
__global__ __launch_bounds__(kThreads) void upgma_update_kernel(UpgmaState* __restrict__ st, double* __restrict__ D, int64_t ld,
                                                                uint64_t* __restrict__ nkey, int32_t* __restrict__ nn, int32_t* __restrict__ list)
{
    const int64_t n = st->n, it = st->it_b, m = n - it;
    const int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (m < 2 || k >= m) return;
    const int64_t x = st->x, y = st->y, last = m - 1;
    const bool moved = y != last;
    if (k == x || k == y) {
        if (k == x) st->it_c = it + 1;
        list[atomicAdd(&st->nres, 1u)] = (int32_t)k;
        return;
    }
    const double val = upgma::merged(st->linkage, st->sx, st->sy, D[x * ld + k], D[y * ld + k]);
    if (k == last && moved) {
        D[x * ld + y] = val;
        D[y * ld + x] = val;
        return;      // the row lives on in slot y, which thread y has listed
    }
    D[x * ld + k] = val;
    D[k * ld + x] = val;
    double dl = 0.0;
    if (moved) {
        dl = D[k * ld + last];
        D[y * ld + k] = D[last * ld + k];
        D[k * ld + y] = dl;
    }
    int32_t cj = nn[k];
    if (cj == x || cj == y) { list[atomicAdd(&st->nres, 1u)] = (int32_t)k; return; }
    uint64_t ck = nkey[k];
    if (moved && cj == last) cj = (int32_t)y;
    cache_take(ck, cj, val, (int32_t)x);
    if (moved) cache_take(ck, cj, dl, (int32_t)y);
    nkey[k] = ck;
    nn[k] = cj;
}

// Reads: st (n, it_c, nres); list[0 .. nres); the rows D[r][0 .. m') of the listed r, m' = n - it_c.  Writes nkey[r], nn[r] of the
// listed rows (thread 0 of the workgroup that took r); thread 0 of workgroup 0 writes st->it_a and adds to st->rescanned, which
// nothing else in the launch reads.  A workgroup takes the entries blockIdx.x, blockIdx.x + gridDim.x, ... (at most m' + 1 of them).
__global__ __launch_bounds__(kRescanThreads) void upgma_rescan_kernel(UpgmaState* __restrict__ st, const double* __restrict__ D, int64_t ld,
                                                                    const int32_t* __restrict__ list, uint64_t* __restrict__ nkey,
                                                                    int32_t* __restrict__ nn, int count_them)
{
    __shared__ uint64_t s_k[kRescanThreads / 64], s_p[kRescanThreads / 64];
    const int64_t m = st->n - st->it_c;
    int64_t nres = st->nres;
    if (nres > m + 1) nres = m + 1;      // the m' + 1 slots of the iteration before, at most
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st->it_a = st->it_c;
        if (count_them && m >= 2) st->rescanned += (unsigned long long)nres;
    }
    if (m < 2) return;
    const int64_t pairs = m >> 1;
    for (int64_t e = blockIdx.x; e < nres; e += gridDim.x) {
        const int64_t r = list[e];
        if (r < 0 || r > m) continue;        // r = m: the slot the merge vacated
        const double* row = D + r * ld;
        uint64_t bk = kNoPair, bp = kNoPair;
        for (int64_t c = threadIdx.x; c < pairs; c += kRescanThreads) {
            const double2 v = reinterpret_cast<const double2*>(row)[c];
            const int64_t j = 2 * c;
            if (j != r) { const uint64_t q = upgma::key(v.x); if (pair_less(q, (uint64_t)j, bk, bp)) { bk = q; bp = (uint64_t)j; } }
            if (j + 1 != r) { const uint64_t q = upgma::key(v.y); if (pair_less(q, (uint64_t)(j + 1), bk, bp)) { bk = q; bp = (uint64_t)(j + 1); } }
        }
        if ((m & 1) && threadIdx.x == 0 && m - 1 != r) {
            const uint64_t q = upgma::key(row[m - 1]);
            if (pair_less(q, (uint64_t)(m - 1), bk, bp)) { bk = q; bp = (uint64_t)(m - 1); }
        }
        __syncthreads();      // the wave entries of the row before this one have been read
        block_min<kRescanThreads>(bk, bp, s_k, s_p);
        if (threadIdx.x == 0) { nkey[r] = bk; nn[r] = (int32_t)bp; }
    }
}

// buffers for n tips (kept when they already hold as many); a copy beyond the device's free memory is refused before any allocation
int upgma_reserve(UpgmaBuffers& B, int64_t n)
{
    if (B.cap_n >= n && B.D) return DPR_OK;
    const int64_t ld = (n + 1) / 2 * 2;      // rows start on 16 bytes
    const size_t need = (size_t)n * (size_t)ld * sizeof(double);
    B.D.reset(); B.size.reset(); B.nkey.reset(); B.nn.reset(); B.list.reset(); B.log_x.reset(); B.log_y.reset(); B.log_h.reset(); B.st.reset();
    B.cap_n = 0;
    size_t free_b = 0, total_b = 0;
    DPR_HIP(hipMemGetInfo(&free_b, &total_b));
    if (need + (size_t)(64 << 20) > free_b) {
        set_error("dpr_upgma_run: the working copy of the matrix over " + std::to_string(n) + " tips needs " + std::to_string(need) +
                  " bytes, the device has " + std::to_string(free_b) + " free");
        return DPR_ERR_ARG;
    }
    const size_t cnt = (size_t)n;
    DPR_HIP(B.D.alloc((size_t)n * (size_t)ld));
    DPR_HIP(B.size.alloc(cnt));
    DPR_HIP(B.nkey.alloc(cnt));
    DPR_HIP(B.nn.alloc(cnt));
    DPR_HIP(B.list.alloc(cnt));
    DPR_HIP(B.log_x.alloc(cnt));
    DPR_HIP(B.log_y.alloc(cnt));
    DPR_HIP(B.log_h.alloc(cnt));
    DPR_HIP(B.st.alloc(sizeof(UpgmaState)));
    B.allocations += 9;
    B.cap_n = n; B.ld = ld;
    return DPR_OK;
}

}  // namespace

}  // namespace dpr

using namespace dpr;

extern "C" {

int64_t dpr_upgma_run(dpr_ctx* c, int linkage, int32_t* merge_x, int32_t* merge_y, double* height)
{
    if (!c || (linkage != 0 && linkage != 1) || !merge_x || !merge_y || !height) {
        set_error("dpr_upgma_run: bad argument (linkage 0 = UPGMA or 1 = WPGMA, no null output)");
        return DPR_ERR_ARG;
    }
    if (c->world > 1 || c->vworld > 0) {
        set_error("dpr_upgma_run: one rank only (no virtual ranks, no several ranks)");
        return DPR_ERR_ARG;
    }
    if (!c->have_matrix) { set_error("dpr_upgma_run: call dpr_dist_matrix first"); return DPR_ERR_STATE; }
    NjBuffers& b0 = c->nj[0];
    const int kind = c->plan.kind;
    if ((kind != DPR_NJ_PLAN_SINGLE_STREAM && kind != DPR_NJ_PLAN_SINGLE_PRUNED && kind != DPR_NJ_PLAN_BIONJ) || b0.pr.sh_world > 1) {
        set_error("dpr_upgma_run: the context's matrix is shared out (virtual shards); one rank on its own whole copy only");
        return DPR_ERR_ARG;
    }
    const int64_t n = b0.N;
    if (n < 2 || n >= ((int64_t)1 << 24)) { set_error("dpr_upgma_run: needs 2 <= n < 2^24 tips"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    NjState nst;
    if (int rc = fetch_state(c, &nst)) return rc;
    if (nst.it != 0 || nst.n != n) {
        set_error("dpr_upgma_run: the matrix is not fresh (" + std::to_string((long long)nst.it) + " NJ iterations since dpr_dist_matrix); build it again");
        return DPR_ERR_STATE;
    }
    UpgmaBuffers& B = c->upgma;
    if (int rc = upgma_reserve(B, n)) return rc;
    B.launches = 0; B.rescanned = 0; B.loop_ms = 0;
    const double* src = b0.D;
    int64_t sld = b0.ld;
    const int32_t* pos = nullptr;
    if (b0.pr.in_positions()) { src = b0.pr.D; sld = b0.pr.ld; pos = b0.pr.pos_of_slot; }
    hipStream_t s = c->stream;
    UpgmaState* st = reinterpret_cast<UpgmaState*>((char*)B.st);
    const int64_t ld = B.ld, cb = (n + kThreads - 1) / kThreads;
    ScopedEvent e0, e1;
    DPR_HIP(hipEventCreate(e0.put()));
    DPR_HIP(hipEventCreate(e1.put()));
    hipLaunchKernelGGL(upgma_fill_kernel, dim3((unsigned)(n * cb)), dim3(kThreads), 0, s, (double*)B.D, ld, n, src, sld, pos, cb);
    hipLaunchKernelGGL(upgma_init_kernel, dim3((unsigned)cb), dim3(kThreads), 0, s, st, (double*)B.size, (int32_t*)B.list, n, linkage);
    hipLaunchKernelGGL(upgma_rescan_kernel, dim3(kRescanBlocks), dim3(kRescanThreads), 0, s, st, (const double*)B.D, ld, (const int32_t*)B.list,
                       (uint64_t*)B.nkey, (int32_t*)B.nn, 0);
    B.launches += 3;
    DPR_HIP(hipGetLastError());
    DPR_HIP(hipEventRecord(e0, s));
    for (int64_t it = 0; it < n - 1; ++it) {
        const int64_t m = n - it;
        hipLaunchKernelGGL(upgma_pick_kernel, dim3(1), dim3(kPickThreads), 0, s, st, (const uint64_t*)B.nkey, (const int32_t*)B.nn, (const double*)B.D,
                           ld, (double*)B.size, (int32_t*)B.log_x, (int32_t*)B.log_y, (double*)B.log_h);
        hipLaunchKernelGGL(upgma_update_kernel, dim3((unsigned)((m + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, st, (double*)B.D, ld,
                           (uint64_t*)B.nkey, (int32_t*)B.nn, (int32_t*)B.list);
        B.launches += 2;
        if (m > 2) {      // after the last merge one slot is left: no cache to keep
            const int64_t blocks = m - 1 < kRescanBlocks ? m - 1 : kRescanBlocks;
            hipLaunchKernelGGL(upgma_rescan_kernel, dim3((unsigned)blocks), dim3(kRescanThreads), 0, s, st, (const double*)B.D, ld,
                               (const int32_t*)B.list, (uint64_t*)B.nkey, (int32_t*)B.nn, 1);
            ++B.launches;
        }
        if ((it & 1023) == 1023) DPR_HIP(hipGetLastError());
    }
    DPR_HIP(hipGetLastError());
    DPR_HIP(hipEventRecord(e1, s));
    UpgmaState hst;
    DPR_HIP(hipMemcpyAsync(merge_x, B.log_x, sizeof(int32_t) * (size_t)(n - 1), hipMemcpyDeviceToHost, s));
    DPR_HIP(hipMemcpyAsync(merge_y, B.log_y, sizeof(int32_t) * (size_t)(n - 1), hipMemcpyDeviceToHost, s));
    DPR_HIP(hipMemcpyAsync(height, B.log_h, sizeof(double) * (size_t)(n - 1), hipMemcpyDeviceToHost, s));
    DPR_HIP(hipMemcpyAsync(&hst, st, sizeof(UpgmaState), hipMemcpyDeviceToHost, s));
    DPR_HIP(hipStreamSynchronize(s));
    float ms = 0;
    DPR_HIP(hipEventElapsedTime(&ms, e0, e1));
    B.loop_ms = ms;
    B.rescanned = (int64_t)hst.rescanned;
    return n - 1;
}

int dpr_upgma_host(const double* lower_rows, int64_t n, int linkage, int32_t* merge_x, int32_t* merge_y, double* height)
{
    if (upgma::run_host(lower_rows, n, linkage, merge_x, merge_y, height)) {
        set_error("dpr_upgma_host: bad argument (2 <= n < 2^24, linkage 0 = UPGMA or 1 = WPGMA, no null pointer)");
        return DPR_ERR_ARG;
    }
    return DPR_OK;
}

int dpr_get_upgma_stats(dpr_ctx* c, int64_t* out4)
{
    if (!c || !out4) { set_error("dpr_get_upgma_stats: bad argument"); return DPR_ERR_ARG; }
    const UpgmaBuffers& B = c->upgma;
    out4[0] = B.D ? (int64_t)(B.cap_n * B.ld * (int64_t)sizeof(double) + B.cap_n * 40 + (int64_t)sizeof(UpgmaState)) : 0;
    out4[1] = B.allocations;
    out4[2] = B.launches;
    out4[3] = B.rescanned;
    return DPR_OK;
}

int dpr_get_upgma_timing(dpr_ctx* c, double* loop_ms)
{
    if (!c) { set_error("dpr_get_upgma_timing: null ctx"); return DPR_ERR_ARG; }
    if (loop_ms) *loop_ms = c->upgma.loop_ms;
    return DPR_OK;
}

}  // extern "C"
