// Each sequence's K nearest neighbours (dpr_nearest_*, include/dipper_hip.h; driver in ctx_nearest.hip; the contract restated on the
// host in nearest_host.hpp).  No reference counterpart.
//
// A block of FULL rows [r0, r0 + nr) x [0, n) lies in memory (row stride ld, a multiple of 16 columns: computed by the source's row
// provider, or expanded from the packed triangle by nearest_expand_kernel, so the select sees one layout).  The order of the contract
// -- smaller distance in fp64, -0.0 == +0.0, then smaller column -- is the order of the pairs (key, j): key = the bits of d (of +0.0
// for either zero) with the sign bit flipped for d >= 0 and all bits flipped for d < 0, compared unsigned.  j is unique in a row, so
// no two candidates compare equal: the K smallest and their order are one answer, whatever way they are found.
//
// nearest_select_kernel: one workgroup of kNearestThreads lanes walks one row in steps of kNearestChunk columns (the first step:
// kNearestThreads columns), a lane loading two pairs of neighbouring columns (16 bytes each, both in flight).  It carries a bound tau =
// the K-th smallest (key, j) at the last cut (everything passes until K are held).  A column survives a step when it is below n, not
// the row itself, finite, and (key, j) < tau: after the first steps almost nothing does.  The survivors of a step go behind the cnt
// candidates held in LDS, at cnt + the survivors of the earlier (load, half, wave) cells of the step (counts in LDS, one barrier a
// step, as pairs_write_kernel) + the lower lanes of the ballot: no atomic, and the place of a candidate in the buffer never matters
// anyway.  At the start of a step with max(2 K, 128) or more candidates held (at most kNearestCap - kNearestChunk = 512, so the step
// always fits), and once as soon as K are held, the workgroup CUTS the buffer back: every lane holds up to kNearestCap /
// kNearestThreads candidates in registers and counts, for each, the candidates that precede it (all lanes read the same candidate: an
// LDS broadcast); the count is its rank, ranks below K go to buffer[rank], tau = buffer[K - 1].  The row ends with one more cut; the
// K places are written in order, d re-read from the row (the entry's own bits, the sign of a zero included), -1 / NaN behind the last
// real one.  Selection by counting costs cnt^2 / kNearestThreads compares a lane and three barriers; a sort network would be cheaper
// above a few hundred candidates and dearer below, where the cuts of real inputs happen (about K ln(n / 256) survivors are expected
// behind the first step of a row in random order).
#include "dpr_internal.hpp"

namespace dpr {

namespace {

constexpr int kNearestWaves = kNearestThreads / 64;
constexpr int kNearestCells = 4 * kNearestWaves;      // (load, half of the load, wave)
constexpr int kNearestHeld = kNearestCap / kNearestThreads;
constexpr int kNearestFirst = kNearestThreads;         // columns of a row's first step: at least kNearestMaxK, even
constexpr int kNearestCutMin = 128;                    // the fewest held candidates that are worth a cut
constexpr int kExpandTile = 64;
static_assert(kNearestCap % kNearestThreads == 0 && kNearestCap - kNearestChunk >= kNearestMaxK, "a selection's K and a step fit");

__device__ inline bool nearest_before(unsigned long long ka, int32_t ja, unsigned long long kb, int32_t jb)
{
    return ka < kb || (ka == kb && ja < jb);
}

struct NearestLds {
    unsigned long long key[kNearestCap];
    int32_t j[kNearestCap];
    unsigned cell[2][kNearestCells];      // [step parity][cell] survivors of a cell
};

// The cnt candidates of the buffer -> the first min(cnt, K) in order at its front; returns that number.  Every lane of the workgroup
// calls it with the same cnt.
__device__ inline int nearest_keep(NearestLds& s, int cnt, int K, int tid)
{
    unsigned long long mk[kNearestHeld];
    int32_t mj[kNearestHeld];
    int rank[kNearestHeld];
    const int held = (cnt + kNearestThreads - 1) / kNearestThreads;      // (the same in every lane)
    __syncthreads();      // (the candidates the other waves wrote in the last step are in the buffer)
#pragma unroll
    for (int q = 0; q < kNearestHeld; ++q) {
        const int e = q * kNearestThreads + tid;
        const bool mine = e < cnt;
        mk[q] = mine ? s.key[e] : ~0ull;
        mj[q] = mine ? s.j[e] : 0x7fffffff;
        rank[q] = 0;
    }
    for (int f = 0; f < cnt; ++f) {
        const unsigned long long kf = s.key[f];
        const int32_t jf = s.j[f];
#pragma unroll
        for (int q = 0; q < kNearestHeld; ++q)
            if (q < held) rank[q] += nearest_before(kf, jf, mk[q], mj[q]) ? 1 : 0;
    }
    __syncthreads();      // (every lane has read the buffer)
#pragma unroll
    for (int q = 0; q < kNearestHeld; ++q) {
        const int e = q * kNearestThreads + tid;
        if (e < cnt && rank[q] < K) { s.key[rank[q]] = mk[q]; s.j[rank[q]] = mj[q]; }      // (ranks are distinct and below cnt <= kNearestCap)
    }
    __syncthreads();
    return cnt < K ? cnt : K;
}

__global__ __launch_bounds__(kNearestThreads) void nearest_select_kernel(const double* __restrict__ rows, int64_t ld, int64_t r0, int64_t n, int K,
                                                                          int32_t* __restrict__ oj, double* __restrict__ od,
                                                                          int32_t* __restrict__ ocnt, int32_t* __restrict__ oflush)
{
    __shared__ NearestLds s;
    const int64_t i = r0 + (int64_t)blockIdx.x;
    const double* row = rows + (int64_t)blockIdx.x * ld;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int cnt = 0, flushes = 0, par = 0;      // (the same in every lane)
    unsigned long long tkey = ~0ull;        // tau: above every finite key until K candidates are held
    int32_t tj = 0x7fffffff;
    // held candidates at which the buffer is cut back to its K best and the bound tightened: a cut costs cnt^2 / kNearestThreads compares
    // a lane, a loose bound lets K / (columns seen at the last cut) of all later columns in.  Never above what leaves room for a step
    const int cut = 2 * K < kNearestCutMin ? kNearestCutMin : 2 * K < kNearestCap - kNearestChunk ? 2 * K : kNearestCap - kNearestChunk;
    // the first step is short (kNearestFirst columns): the K best of it give a bound before the first full step, of which then K /
    // kNearestFirst of the columns survive instead of all
    for (int64_t c0 = 0, width = kNearestFirst; c0 < n; c0 += width, width = kNearestChunk, par ^= 1) {
        if (cnt >= cut || (tkey == ~0ull && cnt >= K)) {
            cnt = nearest_keep(s, cnt, K, tid);
            ++flushes;
            if (cnt == K) { tkey = s.key[K - 1]; tj = s.j[K - 1]; }
        }
        // columns ja, ja + 1 and jb, jb + 1: even, as ld and a step's end are unless that is n, so a pair lies inside the row's ld
        // columns whenever its first column is below the end
        const int64_t end = c0 + width < n ? c0 + width : n;
        const int64_t ja = c0 + 2 * tid, jb = ja + 2 * kNearestThreads;
        double2 va = make_double2(0.0, 0.0), vb = make_double2(0.0, 0.0);
        if (ja < end) va = *reinterpret_cast<const double2*>(row + ja);
        if (jb < end) vb = *reinterpret_cast<const double2*>(row + jb);
        const double v[4] = { va.x, va.y, vb.x, vb.y };
        const int64_t col[4] = { ja, ja + 1, jb, jb + 1 };
        unsigned long long key[4], bal[4];
        bool keep[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            key[q] = nearest_key(v[q]);
            keep[q] = col[q] < end && col[q] != i && nearest_finite(v[q]) && nearest_before(key[q], (int32_t)col[q], tkey, tj);
            bal[q] = __ballot(keep[q]);
        }
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) s.cell[par][q * kNearestWaves + wave] = (unsigned)__popcll(bal[q]);
        }
        __syncthreads();      // (one barrier a step: the next step writes the other parity, the one after it waits behind this barrier's successor)
        unsigned before[4] = { 0, 0, 0, 0 }, total = 0;
#pragma unroll
        for (int c = 0; c < kNearestCells; ++c) {
            const unsigned u = s.cell[par][c];
#pragma unroll
            for (int q = 0; q < 4; ++q) before[q] += c < q * kNearestWaves + wave ? u : 0u;
            total += u;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!keep[q]) continue;
            const int at = cnt + (int)before[q] + __popcll(bal[q] & ((1ull << lane) - 1ull));
            if (at < kNearestCap) { s.key[at] = key[q]; s.j[at] = (int32_t)col[q]; }      // (at < kNearestCap by construction; never a store outside the buffer)
        }
        cnt += (int)total;
        if (cnt > kNearestCap) cnt = kNearestCap;      // (never)
    }
    const int m = nearest_keep(s, cnt, K, tid);
    for (int r = tid; r < K; r += kNearestThreads) {
        const int64_t at = (int64_t)blockIdx.x * K + r;
        const int32_t c = r < m ? s.j[r] : -1;
        const bool real = c >= 0 && c < n;      // (always, for r < m)
        oj[at] = real ? c : -1;
        od[at] = real ? row[c] : __longlong_as_double(0x7ff8000000000000ll);
    }
    if (tid == 0) { ocnt[blockIdx.x] = m; oflush[blockIdx.x] = flushes; }
}

// Rows [r0, r0 + nr) of the packed triangle as full rows.  One workgroup a tile of kExpandTile x kExpandTile: the entries right of the
// diagonal are D_ji = lower[j (j - 1) / 2 + i], contiguous along i -- read with the lanes along i into LDS and written, as the entries
// left of it are read, with the lanes along j (a strided read of the triangle would touch a cache line per entry).
__global__ __launch_bounds__(kNearestThreads) void nearest_expand_kernel(const double* __restrict__ lower, int64_t n, int64_t r0, int64_t nr,
                                                                          double* __restrict__ out, int64_t ld)
{
    __shared__ double tile[kExpandTile][kExpandTile + 1];      // [column][row]
    const int64_t i0 = r0 + (int64_t)blockIdx.y * kExpandTile, j0 = (int64_t)blockIdx.x * kExpandTile;
    const int fast = (int)threadIdx.x & (kExpandTile - 1), slow = (int)threadIdx.x / kExpandTile;
    constexpr int kSlow = kNearestThreads / kExpandTile;
    if (j0 + kExpandTile - 1 > i0) {      // (some column of the tile lies right of some row's diagonal)
        const int64_t i = i0 + fast;
        for (int jj = slow; jj < kExpandTile; jj += kSlow) {
            const int64_t j = j0 + jj;
            if (j > i && j < n && i < r0 + nr) tile[jj][fast] = lower[j * (j - 1) / 2 + i];
        }
    }
    __syncthreads();
    const int64_t j = j0 + fast;
    for (int ii = slow; ii < kExpandTile; ii += kSlow) {
        const int64_t i = i0 + ii;
        if (i >= r0 + nr || j >= n) continue;
        out[(i - r0) * ld + j] = j < i ? lower[i * (i - 1) / 2 + j] : j == i ? 0.0 : tile[fast][ii];
    }
}

}  // namespace

int nearest_expand_packed(const double* lower, int64_t n, int64_t r0, int64_t nr, double* out, int64_t ld, hipStream_t s)
{
    if (nr < 1 || n < 2 || r0 < 0 || r0 + nr > n || ld < n) { set_error("nearest_expand_packed: rows of a block out of range"); return DPR_ERR_ARG; }
    const dim3 grid((unsigned)((n + kExpandTile - 1) / kExpandTile), (unsigned)((nr + kExpandTile - 1) / kExpandTile));
    hipLaunchKernelGGL(nearest_expand_kernel, grid, dim3(kNearestThreads), 0, s, lower, n, r0, nr, out, ld);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

int nearest_select(const double* rows, int64_t ld, int64_t r0, int64_t nr, int64_t n, int K, int32_t* oj, double* od, int32_t* ocnt,
                   int32_t* oflush, hipStream_t s)
{
    if (nr < 1 || nr > kPairsMaxRows || K < 1 || K > kNearestMaxK || n < 2 || ld < n || ld % 2) { set_error("nearest_select: a block out of range"); return DPR_ERR_ARG; }
    hipLaunchKernelGGL(nearest_select_kernel, dim3((unsigned)nr), dim3(kNearestThreads), 0, s, rows, ld, r0, n, K, oj, od, ocnt, oflush);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

}  // namespace dpr
