// Pairs within a distance threshold, and the connected components they form (dpr_pairs_*, include/dipper_hip.h; driver in
// ctx_pairs.hip; the contract restated on the host in pairs_host.hpp).  No reference counterpart.
//
// A row block [r0, r0 + nr) of distances lies in memory (computed by the source's row provider, or the packed triangle in place).
// One workgroup of kPairsThreads lanes walks one row i over its columns j < i in steps of kPairsChunk = 2 kPairsThreads columns; a lane
// looks at columns c0 + lane and c0 + kPairsThreads + lane of a step (coalesced 8-byte loads: the rows of the packed triangle start at
// any multiple of 8 bytes, so there is no wider load that serves both layouts).
//   1. count   pairs_count_kernel: per row the entries with d <= T (NaN and +inf compare false): one 64-bit ballot per sub-step, its
//              population added per wave (the same number in every lane), the waves' sums added through LDS.  One count per row.
//   2. scan    pairs_scan_kernel: one workgroup, exclusive scan of the <= kPairsMaxRows counts in place, total behind them.
//   3. write   pairs_write_kernel: the same walk.  The row's workgroup carries a running base through the row in column order; the
//              place of a kept entry is base + kept entries of the earlier (sub-step, wave) cells of this step (8 counts in LDS) +
//              kept entries of lower lanes in its own ballot.  The order (i, then j) follows from the arithmetic, not from scheduling.
//   4. hook    pairs_hook_kernel: one lane per pair, lock-free union by index: find both roots, atomicCAS(&parent[hi], hi, lo); when
//              the CAS fails the lane goes on from the value it saw.  parent[v] <= v always and a slot is written once by a hook, so
//              every walk descends and ends; no lane waits for a value another lane has yet to write.  pairs_flatten_kernel then
//              writes root(v) for every v (into the forest itself after a block: chains stay short; into the labels at the end).  The
//              root of a component is its smallest index whatever the interleaving of the hooks was.
// The row is walked twice (count, write) rather than the ballots of the count pass kept: a step's 8 ballots are 64 bytes per 4 096 bytes
// read, and a second pass over a block that was just written is served largely from the last-level cache.
#include "dpr_internal.hpp"

namespace dpr {

namespace {

constexpr int kPairsWaves = kPairsThreads / 64;

__device__ inline const double* pairs_row(const double* rows, int64_t ld, int packed, int64_t r0, int64_t i)
{
    return packed ? rows + i * (i - 1) / 2 : rows + (i - r0) * ld;
}

__device__ inline unsigned pairs_lower_lanes(unsigned long long ballot, int lane)
{
    return (unsigned)__popcll(ballot & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kPairsThreads) void pairs_count_kernel(const double* __restrict__ rows, int64_t ld, int packed, int64_t r0, double T,
                                                                     int64_t* __restrict__ cnt)
{
    __shared__ unsigned long long wsum[kPairsWaves];
    const int64_t i = r0 + (int64_t)blockIdx.x;
    const double* row = pairs_row(rows, ld, packed, r0, i);
    const int tid = (int)threadIdx.x, wave = tid >> 6;
    unsigned long long kept = 0;      // of this wave: the same in every lane
    for (int64_t c0 = 0; c0 < i; c0 += kPairsChunk) {      // (i is the same in every lane of the workgroup: every lane reaches every ballot)
        const int64_t j0 = c0 + tid, j1 = j0 + kPairsThreads;
        const bool k0 = j0 < i && row[j0] <= T;
        const bool k1 = j1 < i && row[j1] <= T;
        kept += (unsigned long long)(__popcll(__ballot(k0)) + __popcll(__ballot(k1)));
    }
    if ((tid & 63) == 0) wsum[wave] = kept;
    __syncthreads();
    if (tid == 0) {
        unsigned long long total = 0;
        for (int w = 0; w < kPairsWaves; ++w) total += wsum[w];
        cnt[blockIdx.x] = (int64_t)total;
    }
}

// exclusive scan of cnt[0 .. nr) in place, cnt[nr] = the total.  One workgroup; lane t owns the entries [t * per, (t + 1) * per).
__global__ __launch_bounds__(kPairsThreads) void pairs_scan_kernel(int64_t* __restrict__ cnt, int64_t nr)
{
    __shared__ int64_t part[kPairsThreads];
    const int tid = (int)threadIdx.x;
    const int64_t per = (nr + kPairsThreads - 1) / kPairsThreads;
    const int64_t a = (int64_t)tid * per < nr ? (int64_t)tid * per : nr, b = a + per < nr ? a + per : nr;
    int64_t sum = 0;
    for (int64_t t = a; t < b; ++t) sum += cnt[t];
    part[tid] = sum;
    __syncthreads();
    // Hillis-Steele over the kPairsThreads partial sums (inclusive)
    for (int s = 1; s < kPairsThreads; s <<= 1) {
        const int64_t add = tid >= s ? part[tid - s] : 0;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    int64_t base = part[tid] - sum;
    for (int64_t t = a; t < b; ++t) {
        const int64_t c = cnt[t];
        cnt[t] = base;
        base += c;
    }
    if (tid == kPairsThreads - 1) cnt[nr] = part[tid];
}

__global__ __launch_bounds__(kPairsThreads) void pairs_write_kernel(const double* __restrict__ rows, int64_t ld, int packed, int64_t r0, double T,
                                                                     const int64_t* __restrict__ cnt, int32_t* __restrict__ pi,
                                                                     int32_t* __restrict__ pj, double* __restrict__ pd)
{
    __shared__ unsigned cell[2][2 * kPairsWaves];      // [step parity][sub-step * kPairsWaves + wave] kept entries of a cell
    const int64_t i = r0 + (int64_t)blockIdx.x;
    const double* row = pairs_row(rows, ld, packed, r0, i);
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int64_t base = cnt[blockIdx.x];
    const int64_t end = cnt[blockIdx.x + 1];      // (first pair of the next row, or the block's total)
    int par = 0;
    for (int64_t c0 = 0; c0 < i; c0 += kPairsChunk, par ^= 1) {
        const int64_t j0 = c0 + tid, j1 = j0 + kPairsThreads;
        const double d0 = j0 < i ? row[j0] : 0.0, d1 = j1 < i ? row[j1] : 0.0;
        const bool k0 = j0 < i && d0 <= T;
        const bool k1 = j1 < i && d1 <= T;
        const unsigned long long b0 = __ballot(k0), b1 = __ballot(k1);
        if (lane == 0) { cell[par][wave] = (unsigned)__popcll(b0); cell[par][kPairsWaves + wave] = (unsigned)__popcll(b1); }
        __syncthreads();      // (one barrier a step: the next step writes the other parity, the one after it waits behind this barrier's successor)
        unsigned before0 = 0, before1 = 0, total = 0;
#pragma unroll
        for (int q = 0; q < 2 * kPairsWaves; ++q) {
            const unsigned v = cell[par][q];
            before0 += q < wave ? v : 0u;
            before1 += q < kPairsWaves + wave ? v : 0u;
            total += v;
        }
        if (k0) {
            const int64_t at = base + before0 + pairs_lower_lanes(b0, lane);
            if (at < end) { pi[at] = (int32_t)i; pj[at] = (int32_t)j0; pd[at] = d0; }      // (at < end by construction; never a store outside the row's range)
        }
        if (k1) {
            const int64_t at = base + before1 + pairs_lower_lanes(b1, lane);
            if (at < end) { pi[at] = (int32_t)i; pj[at] = (int32_t)j1; pd[at] = d1; }
        }
        base += total;
    }
}

__device__ inline int32_t pairs_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline int32_t pairs_find(const int32_t* parent, int32_t v)
{
    for (;;) {
        const int32_t p = pairs_load(parent + v);
        if (p == v) return v;
        v = p;      // (p < v: the walk descends)
    }
}

__global__ __launch_bounds__(kPairsThreads) void pairs_hook_kernel(const int32_t* __restrict__ pi, const int32_t* __restrict__ pj, int64_t total,
                                                                    int32_t* parent, int64_t n)
{
    const int64_t p = (int64_t)blockIdx.x * kPairsThreads + threadIdx.x;
    if (p >= total) return;
    int32_t a = pi[p], b = pj[p];
    if (a < 0 || b < 0 || a >= n || b >= n) return;      // (never: the write kernel stores indices below n)
    for (;;) {
        a = pairs_find(parent, a);
        b = pairs_find(parent, b);
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t seen = atomicCAS(parent + hi, hi, lo);
        if (seen == hi) return;
        a = seen; b = lo;      // somebody hooked hi first, under seen < hi: go on from there
    }
}

__global__ __launch_bounds__(kPairsThreads) void pairs_iota_kernel(int32_t* __restrict__ parent, int64_t n)
{
    const int64_t v = (int64_t)blockIdx.x * kPairsThreads + threadIdx.x;
    if (v < n) parent[v] = (int32_t)v;
}

// out[v] = root(v).  out == parent: a slot only ever takes an ancestor of its node, so a walk that reads a slot before or after its
// store ends at the same root
__global__ __launch_bounds__(kPairsThreads) void pairs_flatten_kernel(const int32_t* parent, int32_t* out, int64_t n)
{
    const int64_t v = (int64_t)blockIdx.x * kPairsThreads + threadIdx.x;
    if (v >= n) return;
    const int32_t r = pairs_find(parent, (int32_t)v);
    __hip_atomic_store(out + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

inline unsigned pairs_grid(int64_t items) { return (unsigned)((items + kPairsThreads - 1) / kPairsThreads); }

}  // namespace

int pairs_count_scan(const double* rows, int64_t ld, bool packed, int64_t r0, int64_t nr, double threshold, int64_t* cnt, hipStream_t s)
{
    if (nr < 1 || nr > kPairsMaxRows) { set_error("pairs_count_scan: rows of a block out of range"); return DPR_ERR_ARG; }
    hipLaunchKernelGGL(pairs_count_kernel, dim3((unsigned)nr), dim3(kPairsThreads), 0, s, rows, ld, packed ? 1 : 0, r0, threshold, cnt);
    DPR_HIP(hipGetLastError());
    hipLaunchKernelGGL(pairs_scan_kernel, dim3(1), dim3(kPairsThreads), 0, s, cnt, nr);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

int pairs_write_hook(const double* rows, int64_t ld, bool packed, int64_t r0, int64_t nr, double threshold, const int64_t* cnt, int64_t total,
                     int32_t* pi, int32_t* pj, double* pd, int32_t* parent, int64_t n, hipStream_t s)
{
    if (total <= 0) return DPR_OK;
    hipLaunchKernelGGL(pairs_write_kernel, dim3((unsigned)nr), dim3(kPairsThreads), 0, s, rows, ld, packed ? 1 : 0, r0, threshold, cnt, pi, pj, pd);
    DPR_HIP(hipGetLastError());
    hipLaunchKernelGGL(pairs_hook_kernel, dim3(pairs_grid(total)), dim3(kPairsThreads), 0, s, (const int32_t*)pi, (const int32_t*)pj, total, parent, n);
    DPR_HIP(hipGetLastError());
    return pairs_flatten(parent, parent, n, s);
}

int pairs_hook(const int32_t* pi, const int32_t* pj, int64_t total, int32_t* parent, int64_t n, hipStream_t s)
{
    if (total <= 0) return DPR_OK;
    hipLaunchKernelGGL(pairs_hook_kernel, dim3(pairs_grid(total)), dim3(kPairsThreads), 0, s, pi, pj, total, parent, n);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

int pairs_parent_init(int32_t* parent, int64_t n, hipStream_t s)
{
    hipLaunchKernelGGL(pairs_iota_kernel, dim3(pairs_grid(n)), dim3(kPairsThreads), 0, s, parent, n);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

int pairs_flatten(const int32_t* parent, int32_t* out, int64_t n, hipStream_t s)
{
    hipLaunchKernelGGL(pairs_flatten_kernel, dim3(pairs_grid(n)), dim3(kPairsThreads), 0, s, parent, out, n);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

}  // namespace dpr
