// Transfer bootstrap expectation of NJ trees (Lemoine et al. 2018; no reference counterpart: the reference has no support
// values).
//
// Main internal node n+k has clade A (p = min(|A|, n - |A|)); a replicate tree T* has the clades L_v of all its nodes, leaves
// included.  h = |A| + |L_v| - 2 |A & L_v|, delta = min(h, n - h), phi(A, T*) = min_v delta, in [0, p - 1].
//
// dpr_transfer_support computes phi for every main node with p >= 2 on the device.  Both trees number their leaves in DFS
// order (host, O(n) from the merge logs), so every clade is an interval: [S, E) in main order, [s, e) in replicate order.
// m[t] is the main-order rank of the leaf at replicate position t.  One workgroup takes K main nodes:
//   1. tables   per node and 64-position word w of replicate order: bits = __ballot(S <= m[t] < E) and the exclusive prefix
//               count of the set bits before w (one 16-byte entry: bits lo, bits hi, prefix); each wavefront builds a quarter
//               of the words with a running count, then adds the totals of the quarters before it;
//   2. queries  one lane per replicate INTERNAL node v: |A & L_v| = rank(e) - rank(s), rank(t) = prefix[t >> 6] +
//               popcount(bits[t >> 6] below bit t & 63); the leaves contribute exactly p - 1 (a leaf in A gives h = |A| - 1,
//               one outside gives |A| + 1), so phi = min(p - 1, min over internal v);
//   3. reduce   wavefront min by shuffles, then across the four wavefronts in LDS.
// Work: (n - 2) x (n - 2) node pairs, each two 16-byte LDS reads and two 64-bit popcounts per main node.  The tables take
// K x (n/64 + 1) x 16 bytes of LDS: K = 8 at 30 000 tips (60 KB), 2 at 100 000 (50 KB), 1 up to 655 000 tips; beyond that
// they live in global memory (the same kernel, one table per workgroup of a capped grid), so n is not capped.
//
// dpr_transfer_taxa adds the per-taxon report: the host uploads rep_iv sorted by the canonical key of the
// bipartitions, tbe_kernel<.., true> keeps the place of the closest node with phi, tbe_moved_kernel counts for every tip the
// counted branches whose transfer set holds it; one copy back and one synchronisation for both, as dpr_transfer_support.
//
// dpr_transfer_support_host restates phi without intervals: per main node, |A & L_v| for every replicate node bottom-up in
// merge order, then the min of delta over all of them (leaves included).  dpr_comm_sum_i64 sums the phi over the ranks.
#include "ctx_internal.hpp"
#include "merge_log.hpp"

#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <thread>
#include <type_traits>

namespace dpr {

constexpr int kTbeBatch = 8;                           // words whose m values a wavefront loads before its ballots
constexpr size_t kTbeLdsShared = 64 * 1024;            // default table budget: leaves room for a second workgroup per CU
constexpr size_t kTbeLdsMax = 160 * 1024 - 1024;       // one workgroup per CU (the rest: the kernel's static LDS)
constexpr int64_t kTbeGlobalGrid = 2048;               // workgroups (and tables) of the global-memory variant

// kArg (dpr_transfer_taxa): the minimum is taken over keys delta << 32 | 2 v + (h > n - h), v the node's place in rep_iv, so
// that the smallest v among the closest nodes and the side of its bipartition come out with phi: phi[count + j]
template <int K, bool kLds, bool kArg = false>
__global__ __launch_bounds__(kThreads) void tbe_kernel(const int2* __restrict__ main_iv, int64_t count, const int32_t* __restrict__ m,
                                                       const int2* __restrict__ rep_iv, int64_t n, int64_t nw,
                                                       uint4* __restrict__ scratch, int32_t* __restrict__ phi)
{
    extern __shared__ __attribute__((aligned(16))) uint4 s_tab[];
    constexpr int kWaves = kThreads / 64;
    using Best = std::conditional_t<kArg, uint64_t, int32_t>;
    __shared__ Best s_red[kWaves][K];
    uint4* tab = kLds ? s_tab : scratch + (size_t)blockIdx.x * K * (size_t)nw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t groups = (count + K - 1) / K, seg = (nw + kWaves - 1) / kWaves;
    const int64_t w0 = std::min(nw, wave * seg), w1 = std::min(nw, w0 + seg);
    for (int64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        int S[K], E[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int64_t j = g * K + k;
            const int2 iv = j < count ? main_iv[j] : make_int2(0, 0);     // (padding: an empty clade)
            S[k] = iv.x; E[k] = iv.y;
        }
        // 1. tables: bits and running prefix of this wavefront's words
        uint32_t run[K];
#pragma unroll
        for (int k = 0; k < K; ++k) run[k] = 0;
        for (int64_t wb = w0; wb < w1; wb += kTbeBatch) {
            int mt[kTbeBatch];
#pragma unroll
            for (int b = 0; b < kTbeBatch; ++b) {
                const int64_t t = 64 * (wb + b) + lane;
                mt[b] = (wb + b < w1 && t < n) ? m[t] : -1;
            }
#pragma unroll
            for (int b = 0; b < kTbeBatch; ++b) {
                if (wb + b >= w1) break;                                   // (wavefront-uniform)
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const uint64_t bits = __ballot(S[k] <= mt[b] && mt[b] < E[k]);
                    if (lane == 0) tab[(size_t)k * nw + wb + b] = make_uint4((uint32_t)bits, (uint32_t)(bits >> 32), run[k], 0u);
                    run[k] += (uint32_t)__popcll(bits);
                }
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) s_red[wave][k] = (Best)run[k];
        }
        __syncthreads();
        if (wave > 0) {
            uint32_t off[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                off[k] = 0;
                for (int q = 0; q < wave; ++q) off[k] += (uint32_t)s_red[q][k];
            }
            for (int64_t w = w0 + lane; w < w1; w += 64) {
#pragma unroll
                for (int k = 0; k < K; ++k) tab[(size_t)k * nw + w].z += off[k];
            }
        }
        __syncthreads();
        // 2. queries over the replicate's internal nodes
        Best best[K];
#pragma unroll
        for (int k = 0; k < K; ++k) best[k] = kArg ? (Best)~0ull : (Best)INT_MAX;
        for (int64_t v = threadIdx.x; v < n - 2; v += kThreads) {
            const int2 iv = rep_iv[v];
            const int s = iv.x, e = iv.y;
            const uint64_t ms = (1ull << (s & 63)) - 1, me = (1ull << (e & 63)) - 1;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const uint4 a = tab[(size_t)k * nw + (s >> 6)], b = tab[(size_t)k * nw + (e >> 6)];
                const int rs = (int)a.z + __popcll((((uint64_t)a.y << 32) | a.x) & ms);
                const int re = (int)b.z + __popcll((((uint64_t)b.y << 32) | b.x) & me);
                const int h = (E[k] - S[k]) + (e - s) - 2 * (re - rs);
                if constexpr (kArg)
                    best[k] = std::min(best[k], ((uint64_t)(uint32_t)std::min(h, (int)n - h) << 32) | (uint32_t)(2 * (int)v + (h > (int)n - h)));
                else
                    best[k] = std::min(best[k], std::min(h, (int)n - h));
            }
        }
        // 3. min over the workgroup
#pragma unroll
        for (int k = 0; k < K; ++k)
            for (int o = 32; o > 0; o >>= 1) best[k] = std::min(best[k], __shfl_xor(best[k], o));
        __syncthreads();                                                   // (s_red of step 1 read by every wavefront)
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) s_red[wave][k] = best[k];
        }
        __syncthreads();
        if (threadIdx.x < K) {
            const int64_t j = g * K + threadIdx.x;
            if (j < count) {
                const int2 iv = main_iv[j];
                const int a = iv.y - iv.x, p = std::min(a, (int)n - a);
                if constexpr (kArg) {
                    uint64_t r = ((uint64_t)(uint32_t)(p - 1) << 32) | 0xffffffffu;       // (a leaf: no node of rep_iv)
                    for (int q = 0; q < kWaves; ++q) r = std::min(r, s_red[q][threadIdx.x]);
                    phi[j] = (int32_t)(r >> 32);
                    phi[count + j] = (int32_t)(uint32_t)r;
                } else {
                    int r = p - 1;
                    for (int q = 0; q < kWaves; ++q) r = std::min(r, s_red[q][threadIdx.x]);
                    phi[j] = r;
                }
            }
        }
        __syncthreads();                                                   // (tables and s_red of the next group)
    }
}

// Per-taxon transfer counts (dpr_transfer_taxa).  Branch j is counted when 1000 phi <= cutoff (p - 1); its transfer set is
// A ^ L_v, or the complement of that when h > n - h, v the closest replicate node tbe_kernel<.., true> left in phi_arg.  One
// workgroup takes kMovedTile replicate positions (kMovedPos per thread) and kMovedChunk branches: the chunk's records {S, |A|,
// s, |L_v| + flip << 31} are staged in LDS (a branch that is not counted, or is the root child left out: an empty record, which
// matches no position) and read as broadcasts; a thread tests its positions against every record and adds its non-zero counts
// to moved[t] with one integer atomic each.  Work: listed x n tests of two unsigned range compares.
constexpr int kMovedPos = 4;
constexpr int kMovedTile = kMovedPos * kThreads;
constexpr int kMovedChunk = 1024;

__global__ __launch_bounds__(kThreads) void tbe_moved_kernel(const int2* __restrict__ main_iv, int64_t count, int32_t skip,
                                                             const int32_t* __restrict__ m, const int2* __restrict__ rep_iv, int64_t n,
                                                             const int32_t* __restrict__ phi_arg, int cutoff, int32_t* __restrict__ moved)
{
    __shared__ __attribute__((aligned(16))) uint4 s_rec[kMovedChunk];
    const int64_t j0 = (int64_t)blockIdx.y * kMovedChunk;
    const int chunk = (int)std::min<int64_t>(kMovedChunk, count - j0);
    for (int i = threadIdx.x; i < chunk; i += kThreads) {
        const int64_t j = j0 + i;
        uint4 rec = make_uint4(0u, 0u, 0u, 0u);
        const int2 iv = main_iv[j];
        const int a = iv.y - iv.x, p = std::min(a, (int)n - a);
        const int ph = phi_arg[j], av = phi_arg[count + j];
        if (j != skip && av >= 0 && (av >> 1) < n - 2 && 1000 * (int64_t)ph <= (int64_t)cutoff * (p - 1)) {
            const int2 r = rep_iv[av >> 1];
            rec = make_uint4((uint32_t)iv.x, (uint32_t)a, (uint32_t)r.x, (uint32_t)(r.y - r.x) | ((uint32_t)(av & 1) << 31));
        }
        s_rec[i] = rec;
    }
    uint32_t t[kMovedPos], mt[kMovedPos], cnt[kMovedPos];
#pragma unroll
    for (int q = 0; q < kMovedPos; ++q) {
        const int64_t pos = (int64_t)blockIdx.x * kMovedTile + q * kThreads + threadIdx.x;
        t[q] = (uint32_t)pos;
        mt[q] = pos < n ? (uint32_t)m[pos] : 0xffffffffu;      // (past the end: in no clade; never written)
        cnt[q] = 0;
    }
    __syncthreads();
#pragma unroll 4
    for (int i = 0; i < chunk; ++i) {
        const uint4 rec = s_rec[i];
        const uint32_t len = rec.w & 0x7fffffffu, flip = rec.w >> 31;
#pragma unroll
        for (int q = 0; q < kMovedPos; ++q) cnt[q] += (uint32_t)((mt[q] - rec.x < rec.y) != (t[q] - rec.z < len)) ^ flip;
    }
#pragma unroll
    for (int q = 0; q < kMovedPos; ++q)
        if (t[q] < n && cnt[q]) atomicAdd(&moved[t[q]], (int32_t)cnt[q]);
}

// DFS leaf order of a merge log (merge_log.hpp, the strict rule): the clade of node v (< 2n-2) is [pos[v], pos[v] + size[v]).
struct Dfs : merge_log::Sizes {
    std::vector<int32_t> pos;
};
static bool dfs_of(int64_t n, const int32_t* mx, const int32_t* my, Dfs& d)
{
    if (!merge_log::sizes_of<true>(n, mx, my, d)) return false;
    // the root joins root[0] and root[1]; every other node has a parent with a larger number
    d.pos.assign((size_t)(2 * n - 2), 0);
    d.pos[(size_t)d.root[1]] = d.size[(size_t)d.root[0]];
    for (int64_t it = n - 3; it >= 0; --it) {
        const int32_t v = (int32_t)(n + it), a = d.kid[(size_t)(2 * it)], b = d.kid[(size_t)(2 * it + 1)];
        d.pos[(size_t)a] = d.pos[(size_t)v];
        d.pos[(size_t)b] = d.pos[(size_t)v] + d.size[(size_t)a];
    }
    return true;
}

static bool listed(int64_t n, int32_t size) { return std::min<int64_t>(size, n - size) >= 2; }

// The root's two children name one branch: when both are listed, the k of the one with the larger number (left out of the
// per-taxon counts), else -1.
static int64_t skipped_root_child(int64_t n, const Dfs& d)
{
    const int32_t a = d.root[0], b = d.root[1];
    if (a < n || b < n || !listed(n, d.size[(size_t)a]) || !listed(n, d.size[(size_t)b])) return -1;
    return std::max(a, b) - n;
}

// Canonical key of the bipartition of every internal node n+q of a tree: s = its side without tip 0, key = smallest tip of s
// << 32 | |s| (clades of the tree rooted at tip 0 that share a smallest tip are nested: distinct bipartitions, distinct keys;
// the root's two children share one).  O(n): smallest tips bottom-up, then down the path from the root to tip 0, whose nodes'
// other sides grow by one sibling clade a step.
static std::vector<uint64_t> canonical_keys(int64_t n, const Dfs& d)
{
    const int64_t nodes = 2 * n - 2;
    std::vector<int32_t> low((size_t)nodes), parent((size_t)nodes, -1);
    for (int64_t v = 0; v < n; ++v) low[(size_t)v] = (int32_t)v;
    for (int64_t q = 0; q < n - 2; ++q) {
        const int32_t a = d.kid[(size_t)(2 * q)], b = d.kid[(size_t)(2 * q + 1)];
        low[(size_t)(n + q)] = std::min(low[(size_t)a], low[(size_t)b]);
        parent[(size_t)a] = parent[(size_t)b] = (int32_t)(n + q);
    }
    std::vector<uint64_t> key((size_t)(n - 2));
    for (int64_t q = 0; q < n - 2; ++q) key[(size_t)q] = ((uint64_t)low[(size_t)(n + q)] << 32) | (uint32_t)d.size[(size_t)(n + q)];
    std::vector<int32_t> path;                        // tip 0 up to a root child
    for (int32_t v = 0; v >= 0; v = parent[(size_t)v]) path.push_back(v);
    const int32_t top = path.back();
    int32_t other = low[(size_t)(top == d.root[0] ? d.root[1] : d.root[0])];
    for (size_t i = path.size(); i-- > 0;) {
        const int32_t v = path[i];
        if (v >= n) key[(size_t)(v - n)] = ((uint64_t)other << 32) | (uint32_t)(n - d.size[(size_t)v]);
        if (i > 0) {                                  // the next node down: its sibling's clade joins the other side
            const int32_t a = d.kid[(size_t)(2 * (v - n))], b = d.kid[(size_t)(2 * (v - n) + 1)];
            other = std::min(other, low[(size_t)(a == path[i - 1] ? b : a)]);
        }
    }
    return key;
}

// internal nodes 0 .. n-3 in ascending key order: two stable counting passes (by |s|, then by smallest tip), O(n)
static std::vector<int32_t> canonical_order(int64_t n, const std::vector<uint64_t>& key)
{
    const size_t k = key.size();
    std::vector<int32_t> a(k), b(k), at((size_t)n + 2);
    for (int pass = 0; pass < 2; ++pass) {
        auto digit = [&](int32_t q) { return (size_t)(pass == 0 ? (uint32_t)key[(size_t)q] : (uint32_t)(key[(size_t)q] >> 32)); };
        std::fill(at.begin(), at.end(), 0);
        for (size_t i = 0; i < k; ++i) ++at[digit(pass == 0 ? (int32_t)i : a[i]) + 1];
        for (size_t i = 1; i < at.size(); ++i) at[i] += at[i - 1];
        for (size_t i = 0; i < k; ++i) {
            const int32_t q = pass == 0 ? (int32_t)i : a[i];
            (pass == 0 ? a : b)[(size_t)at[digit(q)]++] = q;
        }
    }
    return b;
}

void tbe_free(TbeBuffers& t)
{
    if (t.main_iv) (void)hipFree(t.main_iv);
    if (t.m) (void)hipFree(t.m);
    if (t.rep_iv) (void)hipFree(t.rep_iv);
    if (t.phi) (void)hipFree(t.phi);
    if (t.scratch) (void)hipFree(t.scratch);
    if (t.phi_arg) (void)hipFree(t.phi_arg);
    if (t.moved) (void)hipFree(t.moved);
    t = TbeBuffers();
}

template <int K, bool kLds, bool kArg = false>
static int tbe_launch(const TbeBuffers& t, int64_t count, int64_t nw, hipStream_t s)
{
    const int64_t groups = (count + K - 1) / K;
    const size_t lds = kLds ? (size_t)K * (size_t)nw * sizeof(uint4) : 0;
    const int64_t grid = kLds ? groups : std::min(groups, kTbeGlobalGrid);
    if (lds > 64 * 1024)
        DPR_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(tbe_kernel<K, kLds, kArg>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((tbe_kernel<K, kLds, kArg>), dim3((unsigned)grid), dim3(kThreads), lds, s, (const int2*)t.main_iv, count,
                       (const int32_t*)t.m, (const int2*)t.rep_iv, t.n, nw, t.scratch, kArg ? t.phi_arg : t.phi);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}

// the per-taxon report of dpr_transfer_taxa (none: dpr_transfer_support)
struct TaxaRequest {
    int cutoff;
    int64_t* moved;
    int64_t* pairs;
};

template <bool kArg>
static int tbe_dispatch(dpr_ctx* c, TbeBuffers& t, int64_t count, int64_t nw)
{
    // nodes per workgroup: the most whose tables fit the budget, else the global-memory variant
    const size_t table = (size_t)nw * sizeof(uint4);
    auto fits = [&](int kk) { return c->tbe_lds > 0 ? (size_t)kk * table <= (size_t)c->tbe_lds
                                                    : ((size_t)kk * table <= kTbeLdsShared || (kk == 1 && table <= kTbeLdsMax)); };
    if (fits(8)) return tbe_launch<8, true, kArg>(t, count, nw, c->stream);
    if (fits(4)) return tbe_launch<4, true, kArg>(t, count, nw, c->stream);
    if (fits(2)) return tbe_launch<2, true, kArg>(t, count, nw, c->stream);
    if (fits(1)) return tbe_launch<1, true, kArg>(t, count, nw, c->stream);
    const size_t need = (size_t)std::min<int64_t>(count, kTbeGlobalGrid) * table;
    if (t.scratch_bytes < need) {
        if (t.scratch) (void)hipFree(t.scratch);
        t.scratch = nullptr; t.scratch_bytes = 0;
        DPR_HIP(hipMalloc(&t.scratch, need));
        t.scratch_bytes = need;
    }
    return tbe_launch<1, false, kArg>(t, count, nw, c->stream);
}

static int transfer_support(dpr_ctx* c, int64_t n, const int32_t* mx, const int32_t* my, const int32_t* rx, const int32_t* ry, int64_t* phi_sum,
                            const TaxaRequest* taxa = nullptr)
{
    TbeBuffers& t = c->tbe;
    const size_t k = (size_t)(n - 2);
    Dfs md, rd;
    const bool same = t.n == n && std::equal(mx, mx + k, t.hx.begin()) && std::equal(my, my + k, t.hy.begin());
    if (!dfs_of(n, rx, ry, rd) || (!same && !dfs_of(n, mx, my, md))) {
        set_error(std::string(taxa ? "dpr_transfer_taxa" : "dpr_transfer_support") + ": not a merge log (0 <= x < y < n - it)");
        return DPR_ERR_ARG;
    }
    const int64_t nw = (n >> 6) + 1;
    if (t.cap < n) {                                    // (buffers for n tips; the main tree is uploaded below)
        tbe_free(t);
        DPR_HIP(hipMalloc(&t.main_iv, sizeof(int2) * k));
        DPR_HIP(hipMalloc(&t.m, sizeof(int32_t) * (size_t)n));
        DPR_HIP(hipMalloc(&t.rep_iv, sizeof(int2) * k));
        DPR_HIP(hipMalloc(&t.phi, sizeof(int32_t) * k));
        t.cap = n;
    }
    if (taxa && t.taxa_cap < n) {
        if (t.phi_arg) (void)hipFree(t.phi_arg);
        if (t.moved) (void)hipFree(t.moved);
        t.phi_arg = t.moved = nullptr; t.taxa_cap = 0;
        DPR_HIP(hipMalloc(&t.phi_arg, sizeof(int32_t) * 2 * k));
        DPR_HIP(hipMalloc(&t.moved, sizeof(int32_t) * (size_t)n));
        t.taxa_cap = n;
    }
    if (!same) {
        std::vector<int2> iv;
        t.n = 0;                                        // (until the upload below has succeeded)
        t.node.clear();
        t.size.clear();
        t.skip = -1;
        const int64_t skip_k = skipped_root_child(n, md);
        for (int64_t q = 0; q < n - 2; ++q) {
            const int32_t sz = md.size[(size_t)(n + q)];
            if (!listed(n, sz)) continue;
            if (q == skip_k) t.skip = (int32_t)t.node.size();
            t.node.push_back((int32_t)q);
            t.size.push_back(sz);
            iv.push_back(make_int2(md.pos[(size_t)(n + q)], md.pos[(size_t)(n + q)] + sz));
        }
        if (!iv.empty()) DPR_HIP(hipMemcpy(t.main_iv, iv.data(), sizeof(int2) * iv.size(), hipMemcpyHostToDevice));
        t.hx.assign(mx, mx + k); t.hy.assign(my, my + k);
        t.n = n;
        t.mpos.assign(md.pos.begin(), md.pos.begin() + n);
    }
    const int64_t count = (int64_t)t.node.size();
    if (count == 0) return DPR_OK;
    std::vector<int32_t> hm((size_t)n);
    std::vector<int2> riv(k);
    for (int64_t leaf = 0; leaf < n; ++leaf) hm[(size_t)rd.pos[(size_t)leaf]] = t.mpos[(size_t)leaf];
    if (taxa) {
        // rep_iv in canonical order of the bipartitions: the smallest place among the closest nodes is then the canonical choice
        const auto t0 = std::chrono::steady_clock::now();
        const std::vector<int32_t> order = canonical_order(n, canonical_keys(n, rd));
        if (log_level("cli"))
            std::fprintf(stderr, "    transfer taxa: canonical order of the replicate's nodes %.3f ms (host)\n",
                         std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        for (size_t i = 0; i < k; ++i) {
            const size_t q = (size_t)order[i];
            riv[i] = make_int2(rd.pos[(size_t)n + q], rd.pos[(size_t)n + q] + rd.size[(size_t)n + q]);
        }
    } else {
        for (size_t q = 0; q < k; ++q) riv[q] = make_int2(rd.pos[(size_t)n + q], rd.pos[(size_t)n + q] + rd.size[(size_t)n + q]);
    }
    DPR_HIP(hipMemcpyAsync(t.m, hm.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    DPR_HIP(hipMemcpyAsync(t.rep_iv, riv.data(), sizeof(int2) * k, hipMemcpyHostToDevice, c->stream));
    int rc = taxa ? tbe_dispatch<true>(c, t, count, nw) : tbe_dispatch<false>(c, t, count, nw);
    if (rc == DPR_OK && taxa) {
        rc = hipMemsetAsync(t.moved, 0, sizeof(int32_t) * (size_t)n, c->stream) == hipSuccess ? DPR_OK : DPR_ERR_HIP;
        if (rc == DPR_OK) {
            const dim3 grid((unsigned)((n + kMovedTile - 1) / kMovedTile), (unsigned)((count + kMovedChunk - 1) / kMovedChunk));
            hipLaunchKernelGGL(tbe_moved_kernel, grid, dim3(kThreads), 0, c->stream, (const int2*)t.main_iv, count, t.skip, (const int32_t*)t.m,
                               (const int2*)t.rep_iv, n, (const int32_t*)t.phi_arg, taxa->cutoff, t.moved);
            if (hipGetLastError() != hipSuccess) rc = DPR_ERR_HIP;
        }
        if (rc == DPR_ERR_HIP) set_error("dpr_transfer_taxa: HIP error");
    }
    if (rc) { (void)hipStreamSynchronize(c->stream); return rc; }     // (the copies above read hm / riv)
    t.hphi.resize((size_t)count);
    DPR_HIP(hipMemcpyAsync(t.hphi.data(), taxa ? t.phi_arg : t.phi, sizeof(int32_t) * (size_t)count, hipMemcpyDeviceToHost, c->stream));
    if (taxa) {
        t.hmoved.resize((size_t)n);
        DPR_HIP(hipMemcpyAsync(t.hmoved.data(), t.moved, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    }
    DPR_HIP(hipStreamSynchronize(c->stream));
    for (int64_t j = 0; j < count; ++j) phi_sum[t.node[(size_t)j]] += t.hphi[(size_t)j];
    if (taxa) {
        // (moved[] per call fits 32 bits: at most one count per listed branch, fewer than 2^30)
        for (int64_t leaf = 0; leaf < n; ++leaf) taxa->moved[leaf] += t.hmoved[(size_t)rd.pos[(size_t)leaf]];
        for (int64_t j = 0; j < count; ++j) {
            if (j == t.skip) continue;
            const int64_t a = t.size[(size_t)j], p = std::min(a, n - a);
            *taxa->pairs += 1000 * (int64_t)t.hphi[(size_t)j] <= (int64_t)taxa->cutoff * (p - 1);
        }
    }
    return DPR_OK;
}

// host restatement: per main node, the intersection with every replicate clade bottom-up, then min of delta over all nodes
static void transfer_host_range(int64_t n, const Dfs& md, const std::vector<int32_t>& leaf_at, const Dfs& rd, int64_t* phi_sum,
                                int64_t first, int64_t step)
{
    std::vector<uint8_t> in((size_t)n, 0);
    std::vector<int32_t> cnt((size_t)(2 * n - 2), 0);
    for (int64_t q = first; q < n - 2; q += step) {
        const int32_t a = md.size[(size_t)(n + q)], S = md.pos[(size_t)(n + q)];
        if (!listed(n, a)) continue;
        for (int32_t i = S; i < S + a; ++i) in[(size_t)leaf_at[(size_t)i]] = 1;
        int64_t best = INT64_MAX;
        for (int64_t v = 0; v < 2 * n - 2; ++v) {
            cnt[(size_t)v] = v < n ? in[(size_t)v] : cnt[(size_t)rd.kid[(size_t)(2 * (v - n))]] + cnt[(size_t)rd.kid[(size_t)(2 * (v - n) + 1)]];
            const int64_t h = (int64_t)a + rd.size[(size_t)v] - 2 * (int64_t)cnt[(size_t)v];
            best = std::min(best, std::min(h, n - h));
        }
        phi_sum[q] += best;
        for (int32_t i = S; i < S + a; ++i) in[(size_t)leaf_at[(size_t)i]] = 0;
    }
}

// host restatement of dpr_transfer_taxa: phi as above; for a counted branch the closest internal node by canonical key, its
// clade marked by a walk over its subtree, and one pass over the tips for the transfer set
static void transfer_taxa_host_range(int64_t n, const Dfs& md, const std::vector<int32_t>& leaf_at, const Dfs& rd,
                                     const std::vector<uint64_t>& key, int64_t skip_k, int cutoff, int64_t* phi_sum, int64_t* moved,
                                     int64_t* pairs, int64_t first, int64_t step)
{
    std::vector<uint8_t> in((size_t)n, 0), inl((size_t)n, 0);
    std::vector<int32_t> cnt((size_t)(2 * n - 2), 0), stack;
    for (int64_t q = first; q < n - 2; q += step) {
        const int32_t a = md.size[(size_t)(n + q)], S = md.pos[(size_t)(n + q)];
        if (!listed(n, a)) continue;
        for (int32_t i = S; i < S + a; ++i) in[(size_t)leaf_at[(size_t)i]] = 1;
        int64_t best = INT64_MAX;
        for (int64_t v = 0; v < 2 * n - 2; ++v) {
            cnt[(size_t)v] = v < n ? in[(size_t)v] : cnt[(size_t)rd.kid[(size_t)(2 * (v - n))]] + cnt[(size_t)rd.kid[(size_t)(2 * (v - n) + 1)]];
            const int64_t h = (int64_t)a + rd.size[(size_t)v] - 2 * (int64_t)cnt[(size_t)v];
            best = std::min(best, std::min(h, n - h));
        }
        phi_sum[q] += best;
        const int64_t p = std::min<int64_t>(a, n - a);
        if (q != skip_k && 1000 * best <= (int64_t)cutoff * (p - 1)) {
            int64_t at = -1;
            bool flip = false;
            for (int64_t v = n; v < 2 * n - 2; ++v) {
                const int64_t h = (int64_t)a + rd.size[(size_t)v] - 2 * (int64_t)cnt[(size_t)v];
                if (std::min(h, n - h) != best || (at >= 0 && key[(size_t)(v - n)] >= key[(size_t)(at - n)])) continue;
                at = v; flip = h > n - h;
            }
            // (phi < p - 1: an internal node reaches the minimum)
            stack.assign(1, (int32_t)at);
            while (!stack.empty()) {
                const int32_t v = stack.back();
                stack.pop_back();
                if (v < n) { inl[(size_t)v] = 1; continue; }
                stack.push_back(rd.kid[(size_t)(2 * (v - n))]);
                stack.push_back(rd.kid[(size_t)(2 * (v - n) + 1)]);
            }
            for (int64_t t = 0; t < n; ++t) {
                moved[t] += (in[(size_t)t] != inl[(size_t)t]) != flip;
                inl[(size_t)t] = 0;
            }
            ++*pairs;
        }
        for (int32_t i = S; i < S + a; ++i) in[(size_t)leaf_at[(size_t)i]] = 0;
    }
}

}  // namespace dpr

using namespace dpr;

extern "C" {

int dpr_transfer_support(dpr_ctx* c, int64_t n, const int32_t* main_x, const int32_t* main_y, const int32_t* rep_x,
                         const int32_t* rep_y, int64_t* phi_sum)
{
    if (!c || n < 2 || n >= ((int64_t)1 << 30) || (n > 2 && (!main_x || !main_y || !rep_x || !rep_y || !phi_sum))) {
        set_error("dpr_transfer_support: bad argument");
        return DPR_ERR_ARG;
    }
    if (n <= 3) return DPR_OK;        // no node with p >= 2
    DPR_HIP(hipSetDevice(c->device));
    const int rc = transfer_support(c, n, main_x, main_y, rep_x, rep_y, phi_sum);
    if (rc == DPR_ERR_HIP) (void)hipGetLastError();
    return rc;
}

int dpr_transfer_support_host(int64_t n, const int32_t* main_x, const int32_t* main_y, const int32_t* rep_x, const int32_t* rep_y,
                              int64_t* phi_sum)
{
    if (n < 2 || n >= ((int64_t)1 << 30) || (n > 2 && (!main_x || !main_y || !rep_x || !rep_y || !phi_sum))) {
        set_error("dpr_transfer_support_host: bad argument");
        return DPR_ERR_ARG;
    }
    if (n <= 3) return DPR_OK;
    Dfs md, rd;
    if (!dfs_of(n, main_x, main_y, md) || !dfs_of(n, rep_x, rep_y, rd)) {
        set_error("dpr_transfer_support_host: not a merge log (0 <= x < y < n - it)");
        return DPR_ERR_ARG;
    }
    std::vector<int32_t> leaf_at((size_t)n);
    for (int64_t leaf = 0; leaf < n; ++leaf) leaf_at[(size_t)md.pos[(size_t)leaf]] = (int32_t)leaf;
    const int64_t hw = std::max<int64_t>(1, (int64_t)std::thread::hardware_concurrency());
    const int64_t T = std::min<int64_t>({ 16, hw, std::max<int64_t>(1, (n - 2) / 256) });
    std::vector<std::thread> pool;
    for (int64_t i = 1; i < T; ++i) pool.emplace_back(transfer_host_range, n, std::cref(md), std::cref(leaf_at), std::cref(rd), phi_sum, i, T);
    transfer_host_range(n, md, leaf_at, rd, phi_sum, 0, T);
    for (auto& th : pool) th.join();
    return DPR_OK;
}

int dpr_transfer_taxa(dpr_ctx* c, int64_t n, const int32_t* main_x, const int32_t* main_y, const int32_t* rep_x, const int32_t* rep_y,
                      int cutoff_permille, int64_t* phi_sum, int64_t* moved, int64_t* pairs)
{
    if (!c || n < 2 || n >= ((int64_t)1 << 30) || cutoff_permille < 0 || cutoff_permille > 999 ||
        (n > 2 && (!main_x || !main_y || !rep_x || !rep_y || !phi_sum || !moved || !pairs))) {
        set_error("dpr_transfer_taxa: bad argument (cutoff: 0 .. 999 per mille)");
        return DPR_ERR_ARG;
    }
    if (n <= 3) return DPR_OK;        // no node with p >= 2
    DPR_HIP(hipSetDevice(c->device));
    const TaxaRequest taxa{ cutoff_permille, moved, pairs };
    const int rc = transfer_support(c, n, main_x, main_y, rep_x, rep_y, phi_sum, &taxa);
    if (rc == DPR_ERR_HIP) (void)hipGetLastError();
    return rc;
}

int dpr_transfer_taxa_host(int64_t n, const int32_t* main_x, const int32_t* main_y, const int32_t* rep_x, const int32_t* rep_y,
                           int cutoff_permille, int64_t* phi_sum, int64_t* moved, int64_t* pairs)
{
    if (n < 2 || n >= ((int64_t)1 << 30) || cutoff_permille < 0 || cutoff_permille > 999 ||
        (n > 2 && (!main_x || !main_y || !rep_x || !rep_y || !phi_sum || !moved || !pairs))) {
        set_error("dpr_transfer_taxa_host: bad argument (cutoff: 0 .. 999 per mille)");
        return DPR_ERR_ARG;
    }
    if (n <= 3) return DPR_OK;
    Dfs md, rd;
    if (!dfs_of(n, main_x, main_y, md) || !dfs_of(n, rep_x, rep_y, rd)) {
        set_error("dpr_transfer_taxa_host: not a merge log (0 <= x < y < n - it)");
        return DPR_ERR_ARG;
    }
    std::vector<int32_t> leaf_at((size_t)n);
    for (int64_t leaf = 0; leaf < n; ++leaf) leaf_at[(size_t)md.pos[(size_t)leaf]] = (int32_t)leaf;
    const std::vector<uint64_t> key = canonical_keys(n, rd);
    const int64_t skip_k = skipped_root_child(n, md);
    const int64_t hw = std::max<int64_t>(1, (int64_t)std::thread::hardware_concurrency());
    const int64_t T = std::min<int64_t>({ 16, hw, std::max<int64_t>(1, (n - 2) / 256) });
    // (every thread counts into arrays of its own; summed below)
    std::vector<std::vector<int64_t>> part((size_t)T, std::vector<int64_t>((size_t)n + 1, 0));
    std::vector<std::thread> pool;
    auto work = [&](int64_t i) {
        transfer_taxa_host_range(n, md, leaf_at, rd, key, skip_k, cutoff_permille, phi_sum, part[(size_t)i].data(), part[(size_t)i].data() + n, i, T);
    };
    for (int64_t i = 1; i < T; ++i) pool.emplace_back(work, i);
    work(0);
    for (auto& th : pool) th.join();
    for (const auto& v : part) {
        for (int64_t t = 0; t < n; ++t) moved[t] += v[(size_t)t];
        *pairs += v[(size_t)n];
    }
    return DPR_OK;
}

int dpr_ctx_set_tbe_lds(dpr_ctx* c, int64_t bytes)
{
    if (!c || bytes < 0 || bytes > (int64_t)kTbeLdsMax) { set_error("dpr_ctx_set_tbe_lds: 0 .. 162816 bytes"); return DPR_ERR_ARG; }
    c->tbe_lds = (int)bytes;
    return DPR_OK;
}

int dpr_comm_sum_i64(dpr_ctx* c, int64_t* host_inout, int64_t count)
{
    if (!c || count < 0 || (count > 0 && !host_inout)) { set_error("dpr_comm_sum_i64: bad argument"); return DPR_ERR_ARG; }
    if (c->world <= 1 || c->vworld > 0 || count == 0) return DPR_OK;     // one rank (or all of them in this context)
    DPR_HIP(hipSetDevice(c->device));
    DevBuf<int64_t> d;
    DPR_HIP(d.alloc((size_t)count));
    int rc = hipMemcpyAsync(d, host_inout, sizeof(int64_t) * (size_t)count, hipMemcpyHostToDevice, c->stream) == hipSuccess ? DPR_OK : DPR_ERR_HIP;
    // (two's complement: the uint64 sum is the int64 sum)
    if (rc == DPR_OK) rc = comm_all_reduce_sum(c, d, (size_t)count, kNcclUint64, c->stream);
    if (rc == DPR_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = DPR_ERR_HIP;
    if (rc == DPR_OK && hipMemcpy(host_inout, d, sizeof(int64_t) * (size_t)count, hipMemcpyDeviceToHost) != hipSuccess) rc = DPR_ERR_HIP;
    if (rc == DPR_ERR_HIP) { (void)hipGetLastError(); set_error("dpr_comm_sum_i64: HIP error"); }
    return rc;
}

}  // extern "C"
