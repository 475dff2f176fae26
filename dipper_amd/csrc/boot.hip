// Felsenstein bootstrap of aligned sequences (no reference counterpart: the reference has no support values).
//
// dpr_msa_resample turns the context's MSA planes into those of replicate r, entirely on the device:
//   1. weights   one thread per draw t: column_t (boot_column, dpr_internal.hpp) and an integer atomicAdd on w[column_t]
//                (order-independent, so bitwise reproducible);
//   2. scan      inclusive scan of w (mi_inclusive_scan, mash_index.hip); start[c] = incl[c] - w[c];
//   3. sources   src[p] = c for p in [start[c], start[c] + w[c]): the replicate alignment is every column, ascending, repeated
//                w[c] times; padding positions p >= L get -1;
//   4. gather    one lane builds one 32-site word of one sequence for X, LO and HI from the uploaded planes; LX = LO | X is
//                derived; padding as msa_planes_kernel (X = 1, LO = HI = 0, LX = 1);
//   5. restage   msa_xstage_kernel on the new planes.  The L-dependent tables (jc_tab) stay valid: a replicate has the same L.
// The planes are then bit for bit those dpr_set_msa builds from the host-written replicate alignment, so every distance
// computed from them is too.  The uploaded alignment's planes stay on the device (MsaBuffers::alt_planes) for replicate -1.
//
// dpr_split_support (host) counts the main tree's splits in a replicate tree from the two merge logs; dpr_comm_sum_i32 sums
// the counts over the ranks.
#include "ctx_internal.hpp"
#include "merge_log.hpp"

#include <algorithm>

namespace dpr {

constexpr int kGatherWords = 64;    // words per gather tile: one per lane of a wavefront
constexpr int kGatherSeqs = 16;     // sequences per tile, 4 per wavefront

__global__ __launch_bounds__(kThreads) void boot_weights_kernel(uint64_t key, int64_t L, int32_t* __restrict__ w)
{
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < L; t += (int64_t)gridDim.x * kThreads)
        atomicAdd(&w[boot_column(key, t, L)], 1);
}

// P = 32 W32 positions: column c < L writes its run of w[c] positions, positions >= L are padding
__global__ __launch_bounds__(kThreads) void boot_sources_kernel(const int32_t* __restrict__ w, const uint32_t* __restrict__ incl,
                                                                int64_t L, int64_t P, int32_t* __restrict__ src)
{
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < P; i += (int64_t)gridDim.x * kThreads) {
        if (i >= L) { src[i] = -1; continue; }
        const int32_t k = w[i];
        const int64_t s0 = (int64_t)incl[i] - k;      // (incl[L - 1] = L: every run ends at or before position L)
        for (int32_t j = 0; j < k; ++j) src[s0 + j] = (int32_t)i;
    }
}

// block: kGatherWords words x kGatherSeqs sequences.  The tile's sources sit in LDS, 33 entries per word, so that the 64 lanes
// reading src[32 lane + b] hit distinct banks.  The sources of one output word are sorted, so its input words are few and
// neighbouring (cache hits).
__global__ __launch_bounds__(kThreads) void boot_gather_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                               const int32_t* __restrict__ src, int64_t n, int64_t W32)
{
    __shared__ int32_t s_src[kGatherWords * 33];
    const int64_t w0 = (int64_t)blockIdx.x * kGatherWords;
    for (int e = threadIdx.x; e < kGatherWords * 32; e += kThreads) {
        const int wl = e >> 5, b = e & 31;
        s_src[wl * 33 + b] = w0 + wl < W32 ? src[(w0 + wl) * 32 + b] : -1;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w = w0 + lane;
    if (w >= W32) return;
    const int64_t groups = (n + kGatherSeqs - 1) / kGatherSeqs;
    for (int64_t g = blockIdx.y; g < groups; g += gridDim.y)
        for (int q = wave; q < kGatherSeqs; q += kThreads / 64) {
            const int64_t s = g * kGatherSeqs + q;
            if (s >= n) break;
            const uint32_t* pX = in + (0 * n + s) * W32;
            const uint32_t* pL = in + (1 * n + s) * W32;
            const uint32_t* pH = in + (2 * n + s) * W32;
            uint32_t x = 0, lo = 0, hi = 0;
            for (int b = 0; b < 32; ++b) {
                const int32_t c = s_src[lane * 33 + b];
                if (c < 0) { x |= 1u << b; continue; }
                const int64_t cw = c >> 5;
                const int sh = c & 31;
                x |= ((pX[cw] >> sh) & 1u) << b;
                lo |= ((pL[cw] >> sh) & 1u) << b;
                hi |= ((pH[cw] >> sh) & 1u) << b;
            }
            out[(0 * n + s) * W32 + w] = x;
            out[(1 * n + s) * W32 + w] = lo;
            out[(2 * n + s) * W32 + w] = hi;
            out[(3 * n + s) * W32 + w] = lo | x;
        }
}

static int msa_resample(MsaBuffers& m, uint64_t seed, int64_t replicate, hipStream_t s)
{
    if (replicate < 0) {                               // back to the uploaded alignment
        if (m.replicate >= 0) { std::swap(m.planes, m.alt_planes); std::swap(m.xstage, m.alt_xstage); m.replicate = -1; }
        return DPR_OK;
    }
    const int64_t L = m.L, P = 32 * m.W32, n = m.n;
    // (first replicate of this upload; each buffer on its own, so that a failed allocation is retried by the next call)
    if (!m.boot_w) DPR_HIP(hipMalloc(&m.boot_w, sizeof(int32_t) * (size_t)L));
    if (!m.boot_incl) DPR_HIP(hipMalloc(&m.boot_incl, sizeof(uint32_t) * (size_t)L));
    if (!m.boot_src) DPR_HIP(hipMalloc(&m.boot_src, sizeof(int32_t) * (size_t)P));
    if (!m.alt_planes) DPR_HIP(hipMalloc(&m.alt_planes, sizeof(uint32_t) * (size_t)(4 * n * m.W32)));
    if (m.xstage && !m.alt_xstage) DPR_HIP(hipMalloc(&m.alt_xstage, sizeof(unsigned long long) * (size_t)n));
    // source = the uploaded planes, target = the replicate buffers (whichever of the two sets holds them now)
    const bool active = m.replicate >= 0;
    const uint32_t* orig = active ? m.alt_planes : m.planes;
    uint32_t* rep = active ? m.planes : m.alt_planes;
    DPR_HIP(hipMemsetAsync(m.boot_w, 0, sizeof(int32_t) * (size_t)L, s));
    const int64_t gl = (L + kThreads - 1) / kThreads, gp = (P + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(boot_weights_kernel, dim3((unsigned)(gl < 8192 ? gl : 8192)), dim3(kThreads), 0, s, boot_key(seed, replicate), L, m.boot_w);
    DPR_HIP(hipGetLastError());
    if (int rc = mi_inclusive_scan(reinterpret_cast<const uint32_t*>(m.boot_w), m.boot_incl, L, s)) return rc;
    hipLaunchKernelGGL(boot_sources_kernel, dim3((unsigned)(gp < 8192 ? gp : 8192)), dim3(kThreads), 0, s, (const int32_t*)m.boot_w,
                       (const uint32_t*)m.boot_incl, L, P, m.boot_src);
    DPR_HIP(hipGetLastError());
    const int64_t groups = (n + kGatherSeqs - 1) / kGatherSeqs;
    const dim3 grid((unsigned)((m.W32 + kGatherWords - 1) / kGatherWords), (unsigned)(groups < 65535 ? groups : 65535));
    hipLaunchKernelGGL(boot_gather_kernel, grid, dim3(kThreads), 0, s, orig, rep, (const int32_t*)m.boot_src, n, m.W32);
    DPR_HIP(hipGetLastError());
    if (!active) { std::swap(m.planes, m.alt_planes); std::swap(m.xstage, m.alt_xstage); }
    m.replicate = replicate;
    if (int rc = msa_restage(m, s)) return rc;
    DPR_HIP(hipStreamSynchronize(s));
    return DPR_OK;
}

// ---- split support (host) ----------------------------------------------------------------------------------------------
// A clade is the XOR of 128-bit tip keys; a split is named by the clade of its side WITHOUT tip 0 (the complement's hash is
// the clade's XOR all tips).  Non-trivial: both sides hold >= 2 tips.  A collision could only inflate a count.
struct Clades {
    std::vector<uint64_t> a, b;     // hash halves of node 0 .. 2n-3 (tips, then the internal nodes in merge order)
    std::vector<int32_t> size;
    std::vector<uint8_t> has0;
    uint64_t ta = 0, tb = 0;        // all tips
};
static bool clades_of(int64_t n, const int32_t* mx, const int32_t* my, Clades& c)
{
    const int64_t nodes = 2 * n - 2;
    c.a.assign((size_t)nodes, 0); c.b.assign((size_t)nodes, 0); c.size.assign((size_t)nodes, 0); c.has0.assign((size_t)nodes, 0);
    c.ta = c.tb = 0;
    for (int64_t t = 0; t < n; ++t) {
        c.a[(size_t)t] = mix64(2 * (uint64_t)t);
        c.b[(size_t)t] = mix64(2 * (uint64_t)t + 1);
        c.size[(size_t)t] = 1;
        c.ta ^= c.a[(size_t)t]; c.tb ^= c.b[(size_t)t];
    }
    c.has0[0] = 1;
    std::vector<int32_t> real;
    return merge_log::replay<true>(n, n - 2, mx, my, real, [&](int64_t, int32_t id, int32_t u, int32_t v) {
        c.a[(size_t)id] = c.a[(size_t)u] ^ c.a[(size_t)v]; c.b[(size_t)id] = c.b[(size_t)u] ^ c.b[(size_t)v];
        c.size[(size_t)id] = c.size[(size_t)u] + c.size[(size_t)v];
        c.has0[(size_t)id] = c.has0[(size_t)u] | c.has0[(size_t)v];
    });
}

}  // namespace dpr

using namespace dpr;

extern "C" {

int dpr_msa_resample(dpr_ctx* c, uint64_t seed, int64_t replicate)
{
    if (!c || replicate < -1) { set_error("dpr_msa_resample: bad argument"); return DPR_ERR_ARG; }
    if (!c->msa.planes) { set_error("dpr_msa_resample: call dpr_set_msa first"); return DPR_ERR_STATE; }
    if (c->msa.aa) { set_error("dpr_msa_resample: bootstrap replicates are not available for a protein alignment (nucleotide alignments only)"); return DPR_ERR_ARG; }
    if (c->msa.L >= ((int64_t)1 << 31)) { set_error("dpr_msa_resample: at most 2^31 - 1 sites"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    const int rc = msa_resample(c->msa, seed, replicate, c->stream);
    if (rc == DPR_ERR_HIP) (void)hipGetLastError();
    return rc;
}

int dpr_get_msa_boot_weights(dpr_ctx* c, int32_t* out)
{
    if (!c || !out) { set_error("dpr_get_msa_boot_weights: bad argument"); return DPR_ERR_ARG; }
    if (!c->msa.planes || c->msa.replicate < 0) { set_error("dpr_get_msa_boot_weights: no replicate is active (dpr_msa_resample)"); return DPR_ERR_STATE; }
    DPR_HIP(hipSetDevice(c->device));
    DPR_HIP(hipStreamSynchronize(c->stream));
    DPR_HIP(hipMemcpy(out, c->msa.boot_w, sizeof(int32_t) * (size_t)c->msa.L, hipMemcpyDeviceToHost));
    return DPR_OK;
}

int dpr_msa_boot_weights(uint64_t seed, int64_t replicate, int64_t L, int32_t* out)
{
    if (!out || replicate < 0 || L < 1 || L >= ((int64_t)1 << 32)) { set_error("dpr_msa_boot_weights: bad argument"); return DPR_ERR_ARG; }
    std::fill(out, out + L, 0);
    const uint64_t key = boot_key(seed, replicate);
    for (int64_t t = 0; t < L; ++t) ++out[boot_column(key, t, L)];
    return DPR_OK;
}

int dpr_split_support(int64_t n, const int32_t* main_x, const int32_t* main_y, const int32_t* rep_x, const int32_t* rep_y, int32_t* counts)
{
    if (n < 2 || n >= ((int64_t)1 << 30) || (n > 2 && (!main_x || !main_y || !rep_x || !rep_y || !counts))) {
        set_error("dpr_split_support: bad argument");
        return DPR_ERR_ARG;
    }
    if (n <= 3) return DPR_OK;        // no non-trivial split
    Clades m, r;
    if (!clades_of(n, main_x, main_y, m) || !clades_of(n, rep_x, rep_y, r)) {
        set_error("dpr_split_support: not a merge log (0 <= x < y < n - it)");
        return DPR_ERR_ARG;
    }
    auto canon = [](const Clades& c, int64_t v, uint64_t& a, uint64_t& b) {
        a = c.a[(size_t)v]; b = c.b[(size_t)v];
        if (c.has0[(size_t)v]) { a ^= c.ta; b ^= c.tb; }
    };
    auto nontrivial = [n](const Clades& c, int64_t v) { return c.size[(size_t)v] >= 2 && c.size[(size_t)v] <= n - 2; };
    // the replicate's splits: an open-addressing set over the internal nodes (the root's two children name one split: a
    // set holds it once)
    size_t cap = 16;
    while (cap < 4 * (size_t)n) cap <<= 1;
    std::vector<uint64_t> ta(cap), tb(cap);
    std::vector<uint8_t> used(cap, 0);
    for (int64_t v = n; v < 2 * n - 2; ++v) {
        if (!nontrivial(r, v)) continue;
        uint64_t a, b;
        canon(r, v, a, b);
        size_t h = (size_t)(a ^ (b >> 7)) & (cap - 1);
        while (used[h] && !(ta[h] == a && tb[h] == b)) h = (h + 1) & (cap - 1);
        used[h] = 1; ta[h] = a; tb[h] = b;
    }
    for (int64_t k = 0; k < n - 2; ++k) {
        const int64_t v = n + k;
        if (!nontrivial(m, v)) continue;
        uint64_t a, b;
        canon(m, v, a, b);
        size_t h = (size_t)(a ^ (b >> 7)) & (cap - 1);
        while (used[h] && !(ta[h] == a && tb[h] == b)) h = (h + 1) & (cap - 1);
        if (used[h]) ++counts[k];
    }
    return DPR_OK;
}

int dpr_comm_sum_i32(dpr_ctx* c, int32_t* host_inout, int64_t count)
{
    if (!c || count < 0 || (count > 0 && !host_inout)) { set_error("dpr_comm_sum_i32: bad argument"); return DPR_ERR_ARG; }
    if (c->world <= 1 || c->vworld > 0 || count == 0) return DPR_OK;     // one rank (or all of them in this context)
    DPR_HIP(hipSetDevice(c->device));
    DevBuf<int32_t> d;
    DPR_HIP(d.alloc((size_t)count));
    int rc = hipMemcpyAsync(d, host_inout, sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, c->stream) == hipSuccess ? DPR_OK : DPR_ERR_HIP;
    if (rc == DPR_OK) rc = comm_all_reduce_sum(c, d, (size_t)count, kNcclInt32, c->stream);
    if (rc == DPR_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = DPR_ERR_HIP;
    if (rc == DPR_OK && hipMemcpy(host_inout, d, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost) != hipSuccess) rc = DPR_ERR_HIP;
    if (rc == DPR_ERR_HIP) { (void)hipGetLastError(); set_error("dpr_comm_sum_i32: HIP error"); }
    return rc;
}

}  // extern "C"
