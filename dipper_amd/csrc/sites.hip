// Complete and partial deletion of gappy alignment sites (no reference counterpart: the reference knows pairwise deletion only).
//
// dpr_msa_filter_sites rewrites the context's planes so that only the columns with enough coverage remain, on the device:
//   1. coverage  cov[c] = sequences whose X bit (plane 0: not a base / not a residue, both alphabets) is 0 at column c.  The X plane
//                is read once, lanes along the word axis (a wavefront reads 256 contiguous bytes of one sequence), gridDim.y and
//                the four wavefronts of a block splitting the sequences.  A thread keeps kCovBits bit-sliced carry-save planes
//                for its word (plane j holds bit j of the 32 column counts) instead of 32 counters, empties them every
//                kCovFlush = 2^kCovBits - 1 sequences into the block's int32 counters in LDS and the block adds those to cov with
//                integer atomicAdd: order-independent, so reproducible.  The kernel counts ~X, which is n - colsum(X) without a
//                second pass; the positions >= L of the last word have X = 1 in every sequence and count 0.
//   2. flags     keep[c] = 1000 cov[c] >= permille n (64-bit integers: a tie is kept); the best coverage for the error message;
//   3. scan      inclusive scan of keep (mi_inclusive_scan, mash_index.hip): L' = incl[L - 1], column c goes to incl[c] - 1;
//   4. sources   src[p] = the p-th kept column for p < L', -1 for L' <= p < 32 W32';
//   5. gather    boot.hip's tile (one lane builds one 32-site output word, the tile's sources in LDS at a stride of 33) with its
//                own input and output widths, for nucleotides (reads X / LO / HI, writes X / LO / HI / LX) and for protein (all
//                six planes); padding as the planes kernels write it (X = 1, the rest 0, LX = LO | X).  The sources of a word
//                ascend but may lie any number of input words apart (a dropped run can be long): the input is indexed per bit;
//   6. derive    jc_tab, xstage and aa_nx from the new planes by the functions the uploads use (msa_derive, msa_aa_derive).
// The context is then bit for bit the one that dpr_set_msa / dpr_set_msa_aa builds from the host-filtered alignment.
#include "ctx_internal.hpp"

#include <algorithm>

namespace dpr {

constexpr int kCovWords = 64;                        // words per coverage block: one per lane of a wavefront
constexpr int kCovWaves = kThreads / 64;             // wavefronts per block, each on sequences of its own
constexpr int kCovBits = 5;                          // carry-save planes per thread
constexpr int kCovFlush = (1 << kCovBits) - 1;       // sequences a thread adds before it empties its planes (31)
constexpr int kCovSeqs = 2 * kCovFlush * kCovWaves;  // sequences per block (gridDim.y = ceil(n / kCovSeqs)): two periods a wavefront
constexpr int kSiteWords = 64;                       // output words per gather tile
constexpr int kSiteSeqs = 16;                        // sequences per gather tile, 4 per wavefront

// X: plane 0, [n][W32].  Block (x, y): words 64 x .. of the sequences y kCovWaves + wave + k gridDim.y kCovWaves.
__global__ __launch_bounds__(kThreads) void sites_coverage_kernel(const uint32_t* __restrict__ X, int64_t n, int64_t W32, int64_t L,
                                                                  int32_t* __restrict__ cov)
{
    __shared__ int32_t s_cnt[kCovWords * 33];      // [word][bit], 33 entries per word: the 64 lanes of a flush hit distinct banks
    for (int e = threadIdx.x; e < kCovWords * 33; e += kThreads) s_cnt[e] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = (int64_t)blockIdx.x * kCovWords + lane;
    if (w < W32) {
        uint32_t c[kCovBits];
#pragma unroll
        for (int j = 0; j < kCovBits; ++j) c[j] = 0u;
        int held = 0;
        auto flush = [&]() {
            for (int b = 0; b < 32; ++b) {
                int v = 0;
#pragma unroll
                for (int j = 0; j < kCovBits; ++j) v |= (int)((c[j] >> b) & 1u) << j;
                if (v) atomicAdd(&s_cnt[lane * 33 + b], v);
            }
#pragma unroll
            for (int j = 0; j < kCovBits; ++j) c[j] = 0u;
            held = 0;
        };
        const int64_t step = (int64_t)gridDim.y * kCovWaves;
        for (int64_t s = (int64_t)blockIdx.y * kCovWaves + wave; s < n; s += step) {
            uint32_t carry = ~X[s * W32 + w];
#pragma unroll
            for (int j = 0; j < kCovBits; ++j) {
                const uint32_t t = c[j] & carry;
                c[j] ^= carry;
                carry = t;
            }
            if (++held == kCovFlush) flush();
        }
        if (held) flush();
    }
    __syncthreads();
    for (int e = threadIdx.x; e < kCovWords * 32; e += kThreads) {
        const int64_t col = ((int64_t)blockIdx.x * kCovWords + (e >> 5)) * 32 + (e & 31);
        const int32_t v = s_cnt[(e >> 5) * 33 + (e & 31)];
        if (col < L && v) atomicAdd(&cov[col], v);
    }
}

__global__ __launch_bounds__(kThreads) void sites_flags_kernel(const int32_t* __restrict__ cov, int64_t L, int64_t n, int permille,
                                                               uint32_t* __restrict__ keep, int32_t* __restrict__ best)
{
    int32_t mx = 0;
    for (int64_t c = (int64_t)blockIdx.x * kThreads + threadIdx.x; c < L; c += (int64_t)gridDim.x * kThreads) {
        const int32_t v = cov[c];
        keep[c] = (int64_t)1000 * v >= (int64_t)permille * n ? 1u : 0u;
        mx = v > mx ? v : mx;
    }
    if (mx) atomicMax(best, mx);
}

// P = 32 W32' positions: kept column c < L writes position incl[c] - 1, positions >= L' = incl[L - 1] are padding
__global__ __launch_bounds__(kThreads) void sites_sources_kernel(const uint32_t* __restrict__ keep, const uint32_t* __restrict__ incl,
                                                                 int64_t L, int64_t Lk, int64_t P, int32_t* __restrict__ src)
{
    const int64_t total = L > P ? L : P;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
        if (i < L && keep[i]) src[(int64_t)incl[i] - 1] = (int32_t)i;      // (incl[i] - 1 < Lk <= P)
        if (i >= Lk && i < P) src[i] = -1;
    }
}

// block: kSiteWords output words x kSiteSeqs sequences; NP planes are read and written ([NP][n][Win] -> [NP][n][Wout], plane 0 = X),
// nucleotides (NP = 3) also write plane 3 = LO | X
template <int NP, bool LX>
__global__ __launch_bounds__(kThreads) void sites_gather_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                                const int32_t* __restrict__ src, int64_t n, int64_t Win, int64_t Wout)
{
    __shared__ int32_t s_src[kSiteWords * 33];
    const int64_t w0 = (int64_t)blockIdx.x * kSiteWords;
    for (int e = threadIdx.x; e < kSiteWords * 32; e += kThreads) {
        const int wl = e >> 5, b = e & 31;
        s_src[wl * 33 + b] = w0 + wl < Wout ? src[(w0 + wl) * 32 + b] : -1;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = w0 + lane;
    if (w >= Wout) return;
    const int64_t groups = (n + kSiteSeqs - 1) / kSiteSeqs;
    for (int64_t g = blockIdx.y; g < groups; g += gridDim.y)
        for (int q = wave; q < kSiteSeqs; q += kThreads / 64) {
            const int64_t s = g * kSiteSeqs + q;
            if (s >= n) break;
            uint32_t v[NP];
#pragma unroll
            for (int p = 0; p < NP; ++p) v[p] = 0u;
            for (int b = 0; b < 32; ++b) {
                const int32_t c = s_src[lane * 33 + b];
                if (c < 0) { v[0] |= 1u << b; continue; }
                const int64_t at = s * Win + (c >> 5);
                const int sh = c & 31;
#pragma unroll
                for (int p = 0; p < NP; ++p) v[p] |= ((in[(int64_t)p * n * Win + at] >> sh) & 1u) << b;
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) out[((int64_t)p * n + s) * Wout + w] = v[p];
            if (LX) out[((int64_t)NP * n + s) * Wout + w] = v[1] | v[0];
        }
}

// cov[L] (device) of the planes of m
static int sites_coverage(const MsaBuffers& m, int32_t* cov, hipStream_t s)
{
    DPR_HIP(hipMemsetAsync(cov, 0, sizeof(int32_t) * (size_t)m.L, s));
    const int64_t gy = (m.n + kCovSeqs - 1) / kCovSeqs;
    const dim3 grid((unsigned)((m.W32 + kCovWords - 1) / kCovWords), (unsigned)(gy < 65535 ? gy : 65535));
    hipLaunchKernelGGL(sites_coverage_kernel, grid, dim3(kThreads), 0, s, (const uint32_t*)m.planes, m.n, m.W32, m.L, cov);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

static void lap_ms(bool on, hipStream_t s, const std::chrono::steady_clock::time_point& t0, double& last, const char* what)
{
    if (!on) return;      // (DPR_LOG=cli: every segment ends with a sync of its own, as msa_upload's)
    (void)hipStreamSynchronize(s);
    const double now = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "  msa_filter_sites: %s %.2f ms (at %.2f)\n", what, now - last, now);
    last = now;
}

// returns L' >= 1 or an error; m is untouched unless 1 <= L' < L
static int64_t sites_filter(MsaBuffers& m, int permille, hipStream_t s)
{
    const bool tlog = log_level("cli") > 0;
    const auto t0 = std::chrono::steady_clock::now();
    double last = 0;
    const int64_t n = m.n, L = m.L, W32 = m.W32;
    DevBuf<int32_t> cov, best, src;
    DevBuf<uint32_t> keep, incl;
    DPR_HIP(cov.alloc((size_t)L));
    DPR_HIP(best.alloc(1));
    DPR_HIP(keep.alloc((size_t)L));
    DPR_HIP(incl.alloc((size_t)L));
    DPR_HIP(src.alloc((size_t)(32 * W32)));
    lap_ms(tlog, s, t0, last, "scratch allocated (5 hipMalloc)");
    if (int rc = sites_coverage(m, cov, s)) return rc;
    lap_ms(tlog, s, t0, last, "coverage kernel");
    DPR_HIP(hipMemsetAsync(best, 0, sizeof(int32_t), s));
    const int64_t gl = (L + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(sites_flags_kernel, dim3((unsigned)(gl < 8192 ? gl : 8192)), dim3(kThreads), 0, s, (const int32_t*)cov, L, n, permille,
                       (uint32_t*)keep, (int32_t*)best);
    DPR_HIP(hipGetLastError());
    if (int rc = mi_inclusive_scan(keep, incl, L, s)) return rc;
    uint32_t kept = 0;
    int32_t h_best = 0;
    DPR_HIP(hipMemcpy(&kept, incl.get() + (L - 1), sizeof(uint32_t), hipMemcpyDeviceToHost));
    DPR_HIP(hipMemcpy(&h_best, best, sizeof(int32_t), hipMemcpyDeviceToHost));
    lap_ms(tlog, s, t0, last, "flags, scan, L' read back");
    const int64_t Lk = kept;
    if (Lk == 0) {
        set_error("dpr_msa_filter_sites: no site has coverage >= " + std::to_string(permille) + " per mille of " + std::to_string(n) +
                  " sequences (best coverage: " + std::to_string(h_best) + " of " + std::to_string(n) + ")");
        return DPR_ERR_ARG;
    }
    if (Lk == L) return L;      // every site kept: nothing is rewritten
    const int64_t Wk = (Lk + 31) / 32, P = 32 * Wk;
    const int64_t tot = L > P ? L : P, gs = (tot + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(sites_sources_kernel, dim3((unsigned)(gs < 8192 ? gs : 8192)), dim3(kThreads), 0, s, (const uint32_t*)keep,
                       (const uint32_t*)incl, L, Lk, P, (int32_t*)src);
    DPR_HIP(hipGetLastError());
    const int np = m.aa ? 6 : 4;
    uint32_t* fresh = nullptr;
    DPR_HIP(hipMalloc(&fresh, sizeof(uint32_t) * (size_t)(np * n * Wk)));
    const int64_t groups = (n + kSiteSeqs - 1) / kSiteSeqs;
    const dim3 grid((unsigned)((Wk + kSiteWords - 1) / kSiteWords), (unsigned)(groups < 65535 ? groups : 65535));
    if (m.aa) hipLaunchKernelGGL((sites_gather_kernel<6, false>), grid, dim3(kThreads), 0, s, (const uint32_t*)m.planes, fresh, (const int32_t*)src, n, W32, Wk);
    else hipLaunchKernelGGL((sites_gather_kernel<3, true>), grid, dim3(kThreads), 0, s, (const uint32_t*)m.planes, fresh, (const int32_t*)src, n, W32, Wk);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { (void)hipFree(fresh); return hip_fail(e, "sites_gather_kernel"); }      // (the uploaded alignment stays)
    lap_ms(tlog, s, t0, last, "sources and gather kernels");
    // the new planes replace the uploaded ones; what depended on L goes (the bootstrap buffers come back with the next replicate)
    (void)hipFree(m.planes);
    m.planes = fresh;
    for (void** p : { (void**)&m.jc_tab, (void**)&m.xstage, (void**)&m.aa_nx, (void**)&m.alt_planes, (void**)&m.alt_xstage, (void**)&m.boot_w,
                      (void**)&m.boot_incl, (void**)&m.boot_src }) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    m.replicate = -1;
    m.L = Lk; m.W32 = Wk;
    int rc = m.aa ? msa_aa_derived_alloc(m) : msa_derived_alloc(m);
    if (rc == DPR_OK) rc = m.aa ? msa_aa_derive(m, s) : msa_derive(m, s);
    if (rc == DPR_OK && hipStreamSynchronize(s) != hipSuccess) rc = hip_fail(hipGetLastError(), "dpr_msa_filter_sites");
    if (rc != DPR_OK) { msa_free(m); return rc; }      // (half a context is none: the next call needs dpr_set_msa*)
    lap_ms(tlog, s, t0, last, "old planes freed, table and xstage rebuilt");
    return Lk;
}

}  // namespace dpr

using namespace dpr;

extern "C" {

int dpr_get_msa_site_coverage(dpr_ctx* c, int32_t* out)
{
    if (!c || !out) { set_error("dpr_get_msa_site_coverage: bad argument"); return DPR_ERR_ARG; }
    if (!c->msa.planes) { set_error("dpr_get_msa_site_coverage: call dpr_set_msa or dpr_set_msa_aa first"); return DPR_ERR_STATE; }
    DPR_HIP(hipSetDevice(c->device));
    DevBuf<int32_t> cov;
    DPR_HIP(cov.alloc((size_t)c->msa.L));
    int rc = sites_coverage(c->msa, cov, c->stream);
    if (rc == DPR_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = DPR_ERR_HIP;
    if (rc == DPR_OK && hipMemcpy(out, cov, sizeof(int32_t) * (size_t)c->msa.L, hipMemcpyDeviceToHost) != hipSuccess) rc = DPR_ERR_HIP;
    if (rc == DPR_ERR_HIP) { (void)hipGetLastError(); set_error("dpr_get_msa_site_coverage: HIP error"); }
    return rc;
}

int64_t dpr_msa_filter_sites(dpr_ctx* c, int permille)
{
    if (!c || permille < 1 || permille > 1000) { set_error("dpr_msa_filter_sites: permille must be 1 .. 1000"); return DPR_ERR_ARG; }
    if (!c->msa.planes) { set_error("dpr_msa_filter_sites: call dpr_set_msa or dpr_set_msa_aa first"); return DPR_ERR_STATE; }
    if (c->msa.replicate >= 0) { set_error("dpr_msa_filter_sites: a bootstrap replicate is active (dpr_msa_resample(seed, -1) first)"); return DPR_ERR_STATE; }
    if (c->msa.L >= ((int64_t)1 << 31)) { set_error("dpr_msa_filter_sites: at most 2^31 - 1 sites"); return DPR_ERR_ARG; }
    if (hipSetDevice(c->device) != hipSuccess) { set_error("dpr_msa_filter_sites: hipSetDevice failed"); return DPR_ERR_HIP; }
    const int64_t rc = sites_filter(c->msa, permille, c->stream);
    if (rc == DPR_ERR_HIP) (void)hipGetLastError();
    return rc;
}

}  // extern "C"
