// Protein alignments behind the aligned-distance entry points of msa.hip (no reference counterpart: the reference's alphabet is
// A/C/G/T).  Definition (include/dipper_hip.h): over the sites where BOTH sequences hold one of the 20 residues (pairwise
// deletion) useful = their number, match = those with equal codes; p = 1 - match / useful; types 1 (p), 2 (JC with 20 states),
// 7 (Poisson), 8 (Kimura 1983).
//
// Device layout: six bit planes per sequence, 32 sites per uint32 word: X (1 = not a residue: code >= 20 or position >= L) and
// the five bits B0..B4 of code + 1 (1..20), all 0 where X.  A not-a-residue site is the 21st symbol 0, so per 32 sites of a pair
//   raw  += popc((B0a^B0b) | (B1a^B1b) | (B2a^B2b) | (B3a^B3b) | (B4a^B4b))     sites whose symbols differ, a one-sided X included
//   both += popc(Xa & Xb)                                                       only in stages where a sequence of the tile has an X
// and with nX[s] = the X positions of sequence s over all words fed:
//   match = sites - raw - both,    useful = sites - nX[a] - nX[b] + both.
// That is 8 integer operations per word pair (five xor, two three-input or, popcount + add) where no sequence of the tile has a
// not-a-residue position in the 16-word stage (MsaBuffers::xstage, as for nucleotides), 10 elsewhere (and, popcount + add).
// The tile is msa.hip's types 1-2 tile: 64 x 64 pairs, 16 x 16 threads, 4 x 4 pairs per thread, 16 words per stage; six planes per
// side are 51 KiB of LDS per workgroup, three workgroups per CU.
#include "dpr_internal.hpp"

namespace dpr {

constexpr int kAaKC = 16;        // plane words (32 sites each) staged per step
constexpr int kAaPlanes = 6;     // X, B0..B4
constexpr int kAaPT = 64;        // pairs per tile edge
constexpr int kAaLDP = kAaPT + 4;

// codes [n][L] bytes -> planes [6][n][W32]; one thread per (sequence, word)
__global__ __launch_bounds__(kThreads) void msa_aa_planes_kernel(const uint8_t* __restrict__ codes, int64_t n, int64_t L, int64_t W32,
                                                                 uint32_t* __restrict__ planes)
{
    const int64_t total = n * W32;
    for (int64_t idx = (int64_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * kThreads) {
        const int64_t s = idx / W32, w = idx % W32;
        uint32_t X = 0, B[5] = { 0, 0, 0, 0, 0 };
        for (int j = 0; j < 32; ++j) {
            const int64_t pos = w * 32 + j;
            const uint32_t c = pos < L ? (uint32_t)codes[s * L + pos] : 255u;
            const uint32_t v = c < 20u ? c + 1u : 0u;
            X |= (v == 0u ? 1u : 0u) << j;
#pragma unroll
            for (int b = 0; b < 5; ++b) B[b] |= ((v >> b) & 1u) << j;
        }
        planes[(0 * n + s) * W32 + w] = X;
#pragma unroll
        for (int b = 0; b < 5; ++b) planes[((int64_t)(1 + b) * n + s) * W32 + w] = B[b];
    }
}

// per sequence: its not-a-residue positions among the 32 W32 of its words, and the stage bits of msa_xstage_kernel (bit j = the
// 16-word stage j holds such a position or a padding word; stages from 63 on share bit 63).  One thread per sequence.
__global__ __launch_bounds__(kThreads) void msa_aa_xstage_kernel(const uint32_t* __restrict__ planes, int64_t n, int64_t W32,
                                                                 unsigned long long* __restrict__ xstage, int32_t* __restrict__ nx)
{
    const int64_t s = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (s >= n) return;
    const int64_t nst = (W32 + kAaKC - 1) / kAaKC;
    unsigned long long bits = (W32 % kAaKC) != 0 ? (1ull << (nst - 1 < 63 ? nst - 1 : 63)) : 0ull;
    int cnt = 0;
    for (int64_t k = 0; k < W32; ++k) {
        const uint32_t x = planes[s * W32 + k];
        if (x != 0u) { const int64_t st = k / kAaKC; bits |= 1ull << (st < 63 ? st : 63); cnt += __popc(x); }
    }
    xstage[s] = bits;
    nx[s] = cnt;
}

__device__ __forceinline__ double msa_aa_epilogue(int useful, int match, int dist_type)
{
    const double p = 1 - double(match) / useful;
    if (dist_type == DPR_DIST_UNCORRECTED) return p;
    if (dist_type == DPR_DIST_JC) return -0.95 * log(1.0 - p / 0.95);
    if (dist_type == DPR_DIST_POISSON) return -log(1.0 - p);
    return -log(1.0 - p - 0.2 * p * p);
}

__device__ __forceinline__ uint32_t aa_or3(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t m;   // (the compiler emits two v_or_b32, see msa.hip)
    asm("v_or3_b32 %0, %1, %2, %3" : "=v"(m) : "v"(a), "v"(b), "v"(c));
    return m;
}

// One 64 x 64 tile: rows s_rid[], columns s_cid[] (-1 = none), output by the TileOut contract of msa.hip's msa_tile (o.tab unused).
__device__ __forceinline__ void msa_aa_tile(const uint32_t* __restrict__ planes, int64_t n, int64_t W32, const int32_t* __restrict__ nx,
                                            int dist_type, const int32_t* s_rid, const int32_t* s_cid, const TileOut& o, char* smem)
{
    constexpr int PT = kAaPT, LDP = kAaLDP;
    typedef uint32_t (*Stage)[kAaKC][LDP];
    Stage sA = reinterpret_cast<Stage>(smem);
    Stage sB = reinterpret_cast<Stage>(smem + sizeof(uint32_t) * kAaPlanes * kAaKC * LDP);
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    int raw[4][4], both[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { raw[r][c] = 0; both[r][c] = 0; }
    // stages in which a sequence of the tile has a not-a-residue position
    __shared__ unsigned long long s_slow;
    unsigned long long slow = ~0ull;
    if (o.xstage) {
        if (tid == 0) s_slow = 0ull;
        __syncthreads();
        if (tid < 2 * PT) {
            const int id = tid < PT ? s_rid[tid] : s_cid[tid - PT];
            const unsigned long long f = id >= 0 ? o.xstage[id] : 0ull;      // (a missing sequence's pairs are never written)
            if (f) atomicOr(&s_slow, f);
        }
        __syncthreads();
        slow = s_slow;
    }
    // staging: thread -> (sequence sq, word quad kq) of every plane of both sides; one 16-byte load per plane
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));
    const int sq = tid >> 2, kq = tid & 3;
    const int64_t ga = s_rid[sq], gb = s_cid[sq];
    int64_t st = 0;
    for (int64_t k0 = 0; k0 < W32; k0 += kAaKC, ++st) {
        const bool fast = !((slow >> (st < 63 ? st : 63)) & 1ull);
        const int64_t k = k0 + 4 * kq;
        const bool whole = k + 3 < W32;
#pragma unroll
        for (int p = fast ? 1 : 0; p < kAaPlanes; ++p) {
            const uint32_t pad = p == 0 ? ~0u : 0u;      // padding and missing sequences = not a residue
            u32x4 va = (u32x4)(pad), vb = (u32x4)(pad);
            if (whole) {
                if (ga >= 0) va = *reinterpret_cast<const u32x4*>(planes + ((int64_t)p * n + ga) * W32 + k);
                if (gb >= 0) vb = *reinterpret_cast<const u32x4*>(planes + ((int64_t)p * n + gb) * W32 + k);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (k + j < W32 && ga >= 0) va[j] = planes[((int64_t)p * n + ga) * W32 + k + j];
                    if (k + j < W32 && gb >= 0) vb[j] = planes[((int64_t)p * n + gb) * W32 + k + j];
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) { sA[p][4 * kq + j][sq] = va[j]; sB[p][4 * kq + j][sq] = vb[j]; }
        }
        __syncthreads();
        auto body = [&](int kk, bool with_x) {
            uint32_t a[kAaPlanes][4], b[kAaPlanes][4];
#pragma unroll
            for (int p = with_x ? 0 : 1; p < kAaPlanes; ++p) {
                const uint4 va = *reinterpret_cast<const uint4*>(&sA[p][kk][ty * 4]);
                const uint4 vb = *reinterpret_cast<const uint4*>(&sB[p][kk][tx * 4]);
                a[p][0] = va.x; a[p][1] = va.y; a[p][2] = va.z; a[p][3] = va.w;
                b[p][0] = vb.x; b[p][1] = vb.y; b[p][2] = vb.z; b[p][3] = vb.w;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint32_t d = aa_or3(a[1][r] ^ b[1][c], a[2][r] ^ b[2][c], a[3][r] ^ b[3][c]);
                    raw[r][c] += __popc(aa_or3(d, a[4][r] ^ b[4][c], a[5][r] ^ b[5][c]));
                    if (with_x) both[r][c] += __popc(a[0][r] & b[0][c]);
                }
        };
        if (fast) {
#pragma unroll 2
            for (int kk = 0; kk < kAaKC; ++kk) body(kk, false);
        } else {
#pragma unroll 2
            for (int kk = 0; kk < kAaKC; ++kk) body(kk, true);
        }
        __syncthreads();
    }
    // every word fed counts, padding words included: they are not-a-residue on both sides and in neither sequence's nx
    const int sites = 32 * kAaKC * (int)((W32 + kAaKC - 1) / kAaKC), padx = sites - 32 * (int)W32;
    int nxa[4], nxb[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int ida = s_rid[ty * 4 + r], idb = s_cid[tx * 4 + r];
        nxa[r] = (ida >= 0 ? nx[ida] : 0) + padx;
        nxb[r] = (idb >= 0 ? nx[idb] : 0) + padx;
    }
    // distances into the LDS tile (row stride PT+1 doubles), then coalesced rows in both orientations
    double* T = reinterpret_cast<double*>(smem);
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int rr = ty * 4 + r, cc = tx * 4 + c;
            double d = 0.0;
            if (rr < o.nr && cc < o.nc && rr + o.diag != cc)
                d = msa_aa_epilogue(sites - nxa[r] - nxb[c] + both[r][c], sites - raw[r][c] - both[r][c], dist_type);
            T[rr * (PT + 1) + cc] = d;
        }
    __syncthreads();
    if (!o.skip_main)
        for (int e = tid; e < PT * PT; e += kThreads) {
            const int rr = e / PT, cc = e % PT;
            if (rr < o.nr && cc < o.nc && (o.lower_base < 0 || o.c_org + cc < o.lower_base + o.r_org + rr))
                o.out[(int64_t)rr * o.ld + cc] = T[rr * (PT + 1) + cc];
        }
    if (o.mir)
        for (int e = tid; e < PT * PT; e += kThreads) {
            const int cc = e / PT, rr = e % PT;
            if (rr < o.nr && cc < o.nc) o.mir[(int64_t)cc * o.mir_ld + rr] = T[rr * (PT + 1) + cc];
        }
}

constexpr size_t msa_aa_tile_lds()
{
    constexpr size_t stage = sizeof(uint32_t) * 2 * kAaPlanes * kAaKC * kAaLDP, tile = sizeof(double) * kAaPT * (kAaPT + 1);
    return stage > tile ? stage : tile;
}

// Matrix front-end, the semantics of msa_dist_kernel: local rows l0.. of (rank, world) (world > 0) or tips row0 + l (world == 0)
// against columns col0 + [0, ncols).  world == 1: only tiles on or below the diagonal are computed and mirrored (the counts are
// symmetric).  transposed: out[(c - col0) * ld + l].
__global__ __launch_bounds__(kThreads, 3) void msa_aa_dist_kernel(const uint32_t* __restrict__ planes, int64_t n, int64_t W32,
                                                                  const int32_t* __restrict__ nx, int dist_type, double* __restrict__ D,
                                                                  int64_t ld, int64_t rows_local, int rank, int world, int64_t row0,
                                                                  int64_t col0, int64_t ncols, int transposed, MsaSparseX xs)
{
    constexpr int PT = kAaPT;
    __shared__ __attribute__((aligned(16))) char smem[msa_aa_tile_lds()];
    __shared__ int32_t s_rid[PT], s_cid[PT];
    const int64_t l0 = (int64_t)blockIdx.y * PT;   // PT divides the ownership block: one owner per row tile
    const int64_t c0 = col0 + (int64_t)blockIdx.x * PT;
    const int64_t g0 = world > 0 ? shard_global_row(l0, rank, world) : row0 + l0;
    const bool mirror = (world == 1);
    if (mirror && c0 > g0 + PT - 1) return;
    if (threadIdx.x < PT) {
        const int64_t ga = g0 + threadIdx.x, gb = c0 + threadIdx.x;
        s_rid[threadIdx.x] = (ga < n && l0 + threadIdx.x < rows_local) ? (int32_t)ga : -1;
        s_cid[threadIdx.x] = (gb < n && gb < col0 + ncols) ? (int32_t)gb : -1;
    }
    __syncthreads();
    TileOut o;
    const int64_t nr = rows_local - l0 < n - g0 ? rows_local - l0 : n - g0;
    const int64_t ncl = col0 + ncols < n ? col0 + ncols : n;
    o.nr = (int)(nr < PT ? nr : PT);
    o.nc = (int)(ncl - c0 < PT ? ncl - c0 : PT);
    o.lower_base = -1; o.r_org = 0; o.c_org = 0;
    o.diag = g0 - c0;
    o.tab = nullptr; o.tab_ld = 0; o.xstage = xs.stage;
    if (transposed) {
        o.skip_main = true; o.out = nullptr; o.ld = 0;
        o.mir = D + (c0 - col0) * ld + l0; o.mir_ld = ld;
    } else {
        o.skip_main = false; o.out = D + l0 * ld + c0; o.ld = ld;
        const bool below = mirror && c0 + PT - 1 < g0;
        o.mir = below ? D + c0 * ld + g0 : nullptr; o.mir_ld = ld;
    }
    msa_aa_tile(planes, n, W32, nx, dist_type, s_rid, s_cid, o, smem);
}

int msa_aa_launch(int dist_type, hipStream_t s, const MsaBuffers& m, double* D, int64_t ld, int64_t rows, int rank, int world,
                  int64_t row0, int64_t col0, int64_t ncols, int transposed)
{
    switch (dist_type) {
    case DPR_DIST_UNCORRECTED: case DPR_DIST_JC: case DPR_DIST_POISSON: case DPR_DIST_KIMURA: break;
    case DPR_DIST_TAJIMANEI: case DPR_DIST_K2P: case DPR_DIST_TAMURA: case DPR_DIST_JINNEI:
        set_error("distance types 3-6 are nucleotide models; a protein alignment takes 1, 2, 7 (Poisson) or 8 (Kimura)");
        return DPR_ERR_ARG;
    default: set_error("unknown distance type for a protein alignment (valid: 1, 2, 7, 8)"); return DPR_ERR_ARG;
    }
    dim3 g((unsigned)((ncols + kAaPT - 1) / kAaPT), (unsigned)((rows + kAaPT - 1) / kAaPT));
    hipLaunchKernelGGL(msa_aa_dist_kernel, g, dim3(kThreads), 0, s, (const uint32_t*)m.planes, m.n, m.W32, (const int32_t*)m.aa_nx, dist_type,
                       D, ld, rows, rank, world, row0, col0, ncols, transposed, MsaSparseX{ m.xstage });
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// test hook: integer counts of one row against columns [0,row), straight from the definition
__global__ __launch_bounds__(kThreads) void msa_aa_counts_row_kernel(const uint32_t* __restrict__ planes, int64_t n, int64_t W32, int64_t row,
                                                                     int32_t* __restrict__ useful, int32_t* __restrict__ match)
{
    const int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (c >= row) return;
    int u = 0, m = 0;
    for (int64_t k = 0; k < W32; ++k) {
        const uint32_t ok = ~planes[row * W32 + k] & ~planes[c * W32 + k];
        uint32_t diff = 0;
        for (int p = 1; p < kAaPlanes; ++p) diff |= planes[((int64_t)p * n + row) * W32 + k] ^ planes[((int64_t)p * n + c) * W32 + k];
        u += __popc(ok);
        m += __popc(ok & ~diff);
    }
    useful[c] = u;
    match[c] = m;
}

int msa_aa_counts_row(const MsaBuffers& m, int64_t row, int32_t* d_useful, int32_t* d_match, hipStream_t s)
{
    if (row <= 0) return DPR_OK;
    const unsigned grid = (unsigned)((row + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(msa_aa_counts_row_kernel, dim3(grid), dim3(kThreads), 0, s, (const uint32_t*)m.planes, m.n, m.W32, row, d_useful, d_match);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// what a protein alignment's planes alone decide: xstage and aa_nx.  msa_aa_derived_alloc allocates them for m.n (both must be
// null), msa_aa_derive fills them from m.planes; msa_aa_upload and the site filter (sites.hip) share the two
int msa_aa_derived_alloc(MsaBuffers& m)
{
    DPR_HIP(hipMalloc(&m.xstage, sizeof(unsigned long long) * (size_t)m.n));
    DPR_HIP(hipMalloc(&m.aa_nx, sizeof(int32_t) * (size_t)m.n));
    return DPR_OK;
}

int msa_aa_derive(MsaBuffers& m, hipStream_t s)
{
    hipLaunchKernelGGL(msa_aa_xstage_kernel, dim3((unsigned)((m.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, (const uint32_t*)m.planes, m.n, m.W32,
                       m.xstage, m.aa_nx);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

int msa_aa_upload(MsaBuffers& m, const uint8_t* codes, int64_t n, int64_t L, hipStream_t s)
{
    msa_free(m);
    m.n = n; m.L = L; m.W32 = (L + 31) / 32; m.aa = true;
    DevBuf<uint8_t> d_in;
    DPR_HIP(d_in.alloc((size_t)(n * L)));
    DPR_HIP(hipMemcpyAsync(d_in, codes, (size_t)(n * L), hipMemcpyHostToDevice, s));
    DPR_HIP(hipMalloc(&m.planes, sizeof(uint32_t) * (size_t)(kAaPlanes * n * m.W32)));
    if (int rc = msa_aa_derived_alloc(m)) return rc;
    const int64_t total = n * m.W32;
    const unsigned grid = (unsigned)((total + kThreads - 1) / kThreads > 8192 ? 8192 : (total + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(msa_aa_planes_kernel, dim3(grid ? grid : 1), dim3(kThreads), 0, s, (const uint8_t*)d_in, n, L, m.W32, m.planes);
    DPR_HIP(hipGetLastError());
    if (int rc = msa_aa_derive(m, s)) return rc;
    DPR_HIP(hipStreamSynchronize(s));      // (d_in is read until here)
    return DPR_OK;
}

}  // namespace dpr
