// C ABI of libdipper_hip.so (see include/dipper_hip.h): the device context, errors and logging, encoders, inputs, sketches,
// measurement aids and test hooks.  The other entry points: ctx_comm.hip (ranks, exchanges), ctx_nj.hip (distance matrix, NJ),
// ctx_place.hip (placement, exact mode, divide-and-conquer).  No CPU fallback: every compute entry point needs a gfx950 device.
#include "ctx_internal.hpp"

namespace dpr {

static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
int log_level(const char* category)
{
    const char* e = std::getenv("DPR_LOG");
    if (!e) return 0;
    const size_t n = std::strlen(category);
    for (const char* p = e; *p;) {
        const char* q = std::strchr(p, ',');
        const size_t len = q ? (size_t)(q - p) : std::strlen(p);
        if (len >= n && std::strncmp(p, category, n) == 0 && (len == n || p[n] == '=')) return len == n ? 1 : std::atoi(p + n + 1);
        if (!q) break;
        p = q + 1;
    }
    return 0;
}
int hip_fail(hipError_t e, const char* what)
{
    // same wording family as the reference's "Gpu_ERROR: ..." messages
    g_err = std::string("Gpu_ERROR: ") + what + ": " + hipGetErrorString(e);
    return DPR_ERR_HIP;
}
const std::string& last_error() { return g_err; }
}  // namespace dpr

using namespace dpr;

__global__ void dpr_warm_kernel(int x) { if (x == 12345) __builtin_trap(); }

extern "C" {

const char* dpr_last_error(void) { return g_err.c_str(); }
int dpr_abi_version(void) { return DPR_ABI_VERSION; }

// ---- encoders (fourBitCompressor / twoBitCompressor semantics) ------------------------------------
static inline uint64_t code_of(char c, uint64_t other)
{
    switch (c) {
    case 'A': return 0;
    case 'C': return 1;
    case 'G': return 2;
    case 'T':
    case 'U': return 3;
    default: return other;
    }
}

int dpr_pack4(const char* seq, uint64_t len, uint64_t* out)
{
    if (!seq || !out) { set_error("dpr_pack4: null argument"); return DPR_ERR_ARG; }
    const uint64_t nw = (len + 15) / 16;
    for (uint64_t w = 0; w < nw; ++w) {
        const uint64_t lo = w * 16, hi = lo + 16 < len ? lo + 16 : len;
        uint64_t v = 0;
        for (uint64_t j = lo; j < hi; ++j) v |= code_of(seq[j], 4) << (4 * (j - lo));
        out[w] = v;
    }
    return DPR_OK;
}

int dpr_pack2(const char* seq, uint64_t len, uint64_t* out)
{
    if (!seq || !out) { set_error("dpr_pack2: null argument"); return DPR_ERR_ARG; }
    const uint64_t nw = (len + 31) / 32;
    for (uint64_t w = 0; w < nw; ++w) {
        const uint64_t lo = w * 32, hi = lo + 32 < len ? lo + 32 : len;
        uint64_t v = 0;
        for (uint64_t j = lo; j < hi; ++j) v |= code_of(seq[j], 0) << (2 * (j - lo));
        out[w] = v;
    }
    return DPR_OK;
}

// amino acids: ARNDCQEGHILKMFPSTWYV -> 0..19 in either case, everything else 255
int dpr_pack_aa(const char* seq, uint64_t len, uint8_t* out)
{
    if ((!seq || !out) && len) { set_error("dpr_pack_aa: null argument"); return DPR_ERR_ARG; }
    static const char kLetters[] = "ARNDCQEGHILKMFPSTWYV";
    uint8_t table[256];
    for (int i = 0; i < 256; ++i) table[i] = 255;
    for (int i = 0; i < 20; ++i) { table[(unsigned char)kLetters[i]] = (uint8_t)i; table[(unsigned char)(kLetters[i] + 32)] = (uint8_t)i; }
    for (uint64_t j = 0; j < len; ++j) out[j] = table[(unsigned char)seq[j]];
    return DPR_OK;
}

// ---- sharding helpers -------------------------------------------------------------------------------
int dpr_njr_owner(int64_t position, int world) { return world > 0 && position >= 0 ? njr_owner(position, world) : -1; }
int64_t dpr_njr_local_row(int64_t position, int world) { return world > 0 && position >= 0 ? njr_local_row(position, world) : -1; }
int64_t dpr_njr_global_pos(int64_t local_row, int rank, int world) { return world > 0 && local_row >= 0 ? njr_global_pos(local_row, rank, world) : -1; }
int64_t dpr_njr_rows_cap(int64_t positions, int world) { return world > 0 && positions >= 0 ? njr_rows_cap(positions, world) : -1; }
int dpr_shard_owner(int64_t row, int world) { return shard_owner(row, world); }
int64_t dpr_shard_local_row(int64_t row, int world) { return shard_local_row(row, world); }
int64_t dpr_shard_rows(int64_t n, int rank, int world) { return shard_rows(n, rank, world); }
int64_t dpr_shard_global_row(int64_t local, int rank, int world) { return shard_global_row(local, rank, world); }
uint64_t dpr_nj_key(int64_t i, int64_t j, int64_t n) { return nj_key_a(i, n) | nj_key_b(j); }

int dpr_record_reduce(const void* records, int count)
{
    const NjRecord* r = (const NjRecord*)records;
    int best = -1;
    for (int i = 0; i < count; ++i) {
        if (r[i].key == ~0ull) continue;
        if (best < 0 || r[i].q < r[best].q || (r[i].q == r[best].q && r[i].key < r[best].key)) best = i;
    }
    return best;
}

// ---- context ----------------------------------------------------------------------------------------
int dpr_create(dpr_ctx** out, int device)
{
    if (!out) { set_error("dpr_create: null out"); return DPR_ERR_ARG; }
    *out = nullptr;
    const bool tlog = log_level("cli") > 0;
    const auto tc0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (tlog) std::fprintf(stderr, "  dpr_create: %s at %.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tc0).count());
    };
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    lap("hipGetDeviceCount (runtime start-up)");
    if (e != hipSuccess || count <= 0) {
        set_error("Gpu_ERROR: no HIP device available (this library has no CPU fallback)");
        return DPR_ERR_HIP;
    }
    if (device < 0 || device >= count) { set_error("dpr_create: device index out of range"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    DPR_HIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error(std::string("Gpu_ERROR: device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
        return DPR_ERR_HIP;
    }
    lap("hipSetDevice + properties");
    dpr_ctx* c = new dpr_ctx();
    c->device = device;
    hipError_t ce = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (auto& ev : c->ev)
        if (ce == hipSuccess) ce = hipEventCreate(&ev);
    if (ce != hipSuccess) {          // nothing of a half-built context is left behind
        for (auto& ev : c->ev) if (ev) (void)hipEventDestroy(ev);
        if (c->stream) (void)hipStreamDestroy(c->stream);
        delete c;
        return hip_fail(ce, "dpr_create: stream / event creation");
    }
    // first launch of the library: the runtime loads the whole gfx950 code object now, i.e. inside context creation
    // (which the CLI overlaps with reading the input) instead of in front of the first distance kernel
    lap("stream + events");
    hipLaunchKernelGGL(dpr_warm_kernel, dim3(1), dim3(64), 0, c->stream, 0);
    (void)hipGetLastError();
    if (tlog) { (void)hipStreamSynchronize(c->stream); lap("first kernel (code object load) done"); }

    *out = c;
    return DPR_OK;
}

int dpr_destroy(dpr_ctx* c)
{
    if (!c) return DPR_OK;
    const bool tlog = log_level("cli") > 0;
    const auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (tlog) std::fprintf(stderr, "  dpr_destroy: %s at %.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    };
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
    shm_comm_free(c);
    for (hipEvent_t e : c->nj_kt.ev) (void)hipEventDestroy(e);
    lap("events destroyed");
    for (auto& b : c->nj) nj_free(b);
    lap("NJ buffers freed");
    msa_free(c->msa);
    mash_free(c->mash);
    place_free(c->place);
    exact_free(c->exact);
    pfix_free(c->pfix);
    tbe_free(c->tbe);
    c->pairs.reset();
    c->nearest.reset();
    c->mst.reset();
    if (c->place_trace) (void)hipFree(c->place_trace);
    if (c->packed_lower) (void)hipFree(c->packed_lower);
    for (auto& ev : c->ev) if (ev) (void)hipEventDestroy(ev);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    lap("other buffers freed");
    if (c->stream) (void)hipStreamDestroy(c->stream);
    lap("streams destroyed");
    delete c;
    return DPR_OK;
}

int dpr_create_virtual(dpr_ctx** out, int device, int world)
{
    if (world < 1 || world > 64) { set_error("dpr_create_virtual: world out of range"); return DPR_ERR_ARG; }
    if (int rc = dpr_create(out, device)) return rc;
    dpr_ctx* c = *out;
    c->world = world;
    c->vworld = world > 1 ? world : 0;
    c->nj = std::vector<NjBuffers>((size_t)world);
    return DPR_OK;
}

int dpr_device_name(dpr_ctx* c, char* buf, int cap)
{
    if (!c || !buf || cap <= 0) { set_error("dpr_device_name: bad argument"); return DPR_ERR_ARG; }
    hipDeviceProp_t prop;
    DPR_HIP(hipGetDeviceProperties(&prop, c->device));
    std::snprintf(buf, (size_t)cap, "%s (%s, %d CUs)", prop.name, prop.gcnArchName, prop.multiProcessorCount);
    return DPR_OK;
}

// ---- inputs ------------------------------------------------------------------------------------------
int dpr_set_msa(dpr_ctx* c, const uint64_t* packed4, int64_t n, int64_t L)
{
    if (!c || !packed4 || n < 2 || L < 1) { set_error("dpr_set_msa: bad argument"); return DPR_ERR_ARG; }
    if (n >= (1 << 24)) { set_error("dpr_set_msa: n must be < 2^24"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    c->n_input = n;
    return msa_upload(c->msa, packed4, n, L, c->stream);
}

int dpr_set_msa_aa(dpr_ctx* c, const uint8_t* codes, int64_t n, int64_t L)
{
    if (!c || !codes || n < 2 || L < 1) { set_error("dpr_set_msa_aa: bad argument"); return DPR_ERR_ARG; }
    if (n >= (1 << 24)) { set_error("dpr_set_msa_aa: n must be < 2^24"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    c->n_input = n;
    return msa_aa_upload(c->msa, codes, n, L, c->stream);
}

int dpr_set_reads(dpr_ctx* c, const uint64_t* packed2, const uint64_t* word_off, const uint64_t* len, int64_t n)
{
    if (!c || !packed2 || !word_off || !len || n < 2) { set_error("dpr_set_reads: bad argument"); return DPR_ERR_ARG; }
    if (n >= (1 << 24)) { set_error("dpr_set_reads: n must be < 2^24"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    c->n_input = n;
    return mash_upload(c->mash, packed2, word_off, len, n, c->stream);
}

int dpr_set_matrix_lower(dpr_ctx* c, const double* rows, int64_t n)
{
    if (!c || !rows || n < 2) { set_error("dpr_set_matrix_lower: bad argument"); return DPR_ERR_ARG; }
    if (n >= (1 << 24)) { set_error("dpr_set_matrix_lower: n must be < 2^24"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    if (c->packed_lower) { (void)hipFree(c->packed_lower); c->packed_lower = nullptr; }
    const size_t cnt = (size_t)(n * (n - 1) / 2);
    DPR_HIP(hipMalloc(&c->packed_lower, sizeof(double) * (cnt ? cnt : 1)));
    DPR_HIP(hipMemcpyAsync(c->packed_lower, rows, sizeof(double) * cnt, hipMemcpyHostToDevice, c->stream));
    DPR_HIP(hipStreamSynchronize(c->stream));
    c->n_input = n;
    return DPR_OK;
}

int dpr_sketch(dpr_ctx* c, int k, int S, uint64_t* host_sketches)
{
    if (!c || !c->mash.packed2) { set_error("dpr_sketch: call dpr_set_reads first"); return DPR_ERR_STATE; }
    DPR_HIP(hipSetDevice(c->device));
    if (int rc = mash_sketch(c->mash, k, S, c->stream)) return rc;
    DPR_HIP(hipStreamSynchronize(c->stream));
    if (host_sketches)
        DPR_HIP(hipMemcpy(host_sketches, c->mash.sketches, sizeof(uint64_t) * (size_t)(c->mash.n * S), hipMemcpyDeviceToHost));
    return DPR_OK;
}

int dpr_get_mash_index_info(dpr_ctx* c, int64_t info[8])
{
    if (!c || !info) { set_error("dpr_get_mash_index_info: null argument"); return DPR_ERR_ARG; }
    if (!c->mash.sketches) { set_error("dpr_get_mash_index_info: call dpr_set_reads and dpr_sketch first"); return DPR_ERR_STATE; }
    mash_index_info(c->mash.index, info);
    return DPR_OK;
}

int dpr_get_kmer_hashes(dpr_ctx* c, int64_t seq, int k, const uint64_t* word_off, const uint64_t* len, uint64_t* out)
{
    if (!c || !c->mash.packed2 || seq < 0 || seq >= c->mash.n || !out || k < 1 || k > 15) { set_error("dpr_get_kmer_hashes: bad argument"); return DPR_ERR_ARG; }
    const uint64_t L = len[seq];
    if (L < (uint64_t)k) return DPR_OK;
    const uint64_t nk = L - (uint64_t)k + 1;
    DevBuf<uint64_t> d;
    DPR_HIP(d.alloc(nk));
    if (int rc = mash_hash_positions(c->mash, seq, k, d, L, word_off[seq], c->stream)) return rc;
    DPR_HIP(hipStreamSynchronize(c->stream));
    DPR_HIP(hipMemcpy(out, d, sizeof(uint64_t) * nk, hipMemcpyDeviceToHost));
    return DPR_OK;
}

// microbenchmark: wall time per launch of a chain of trivial dependent kernels (eager or graph replay)
__global__ void dpr_nop_kernel(unsigned long long* p) { if (threadIdx.x == 0 && blockIdx.x == 0 && p[7] == 12345) p[6] = 1; }

__global__ void dpr_mark_kernel(unsigned long long* out, long long idx) { if (threadIdx.x == 0 && blockIdx.x == 0) out[idx] = (unsigned long long)idx + 1ull; }

int dpr_launch_bench(dpr_ctx* c, int nlaunch, int grid, int use_graph, float* us_per_launch)
{
    if (!c || nlaunch < 1 || grid < 1 || !us_per_launch) { set_error("dpr_launch_bench: bad argument"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    DevBuf<unsigned long long> buf;
    DPR_HIP(buf.alloc(8));
    DPR_HIP(hipMemset(buf, 0, 64));
    ScopedGraph g_keep;       // use_graph == 2 (the node handles live in the graph: it stays until the replays are done)
    ScopedGraphExec ge;
    const int per = 128;
    if (use_graph) {
        ScopedGraph g;
        DPR_HIP(hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
        for (int k = 0; k < per; ++k) hipLaunchKernelGGL(dpr_nop_kernel, dim3(grid), dim3(256), 0, c->stream, buf);
        DPR_HIP(hipStreamEndCapture(c->stream, g.put()));
        DPR_HIP(hipGraphInstantiate(ge.put(), g, nullptr, nullptr, 0));
    }
    // use_graph == 2: an explicitly built chain whose nodes get NEW PARAMETERS (argument and grid) before every replay --
    // what a loop with per-launch arguments (placement: the tip index, the distance row) would have to do to be replayed
    std::vector<hipGraphNode_t> nodes;
    DevBuf<unsigned long long> marks;             // use_graph == 2: launch i writes marks[i] = i + 1 (every launch must see ITS parameters)
    if (use_graph == 2) {
        DPR_HIP(marks.alloc((size_t)nlaunch));
        DPR_HIP(hipMemset(marks, 0, sizeof(unsigned long long) * (size_t)nlaunch));
    }
    unsigned long long* argp = marks;
    long long argi = 0;
    void* kargs[2] = { &argp, &argi };
    if (use_graph == 2) {
        ge.reset();
        DPR_HIP(hipGraphCreate(g_keep.put(), 0));
        for (int k = 0; k < per; ++k) {
            hipKernelNodeParams kp{};
            kp.func = reinterpret_cast<void*>(dpr_mark_kernel);
            kp.gridDim = dim3((unsigned)grid); kp.blockDim = dim3(256); kp.sharedMemBytes = 0; kp.kernelParams = kargs; kp.extra = nullptr;
            hipGraphNode_t nd = nullptr;
            DPR_HIP(hipGraphAddKernelNode(&nd, g_keep, k ? &nodes.back() : nullptr, k ? 1 : 0, &kp));
            nodes.push_back(nd);
        }
        DPR_HIP(hipGraphInstantiate(ge.put(), g_keep, nullptr, nullptr, 0));
    }
    DPR_HIP(hipStreamSynchronize(c->stream));
    DPR_HIP(hipEventRecord(c->ev[2], c->stream));
    int done = 0;
    if (use_graph == 2) {
        for (; done + per <= nlaunch; done += per) {
            for (int k = 0; k < per; ++k) {
                hipKernelNodeParams kp{};
                kp.func = reinterpret_cast<void*>(dpr_mark_kernel);
                argi = (long long)(done + k);
                kp.gridDim = dim3((unsigned)(grid + ((done / per + k) & 1))); kp.blockDim = dim3(256); kp.sharedMemBytes = 0; kp.kernelParams = kargs; kp.extra = nullptr;
                DPR_HIP(hipGraphExecKernelNodeSetParams(ge, nodes[(size_t)k], &kp));
            }
            DPR_HIP(hipGraphLaunch(ge, c->stream));
        }
    } else if (use_graph) for (; done + per <= nlaunch; done += per) DPR_HIP(hipGraphLaunch(ge, c->stream));
    for (; done < nlaunch; ++done) hipLaunchKernelGGL(dpr_nop_kernel, dim3(grid), dim3(256), 0, c->stream, buf);
    DPR_HIP(hipEventRecord(c->ev[3], c->stream));
    DPR_HIP(hipStreamSynchronize(c->stream));
    float ms = 0;
    DPR_HIP(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    *us_per_launch = ms * 1e3f / (float)nlaunch;
    int rc_marks = DPR_OK;
    if (marks) {
        std::vector<unsigned long long> h((size_t)done);
        if (done > 0 && hipMemcpy(h.data(), marks, sizeof(unsigned long long) * (size_t)done, hipMemcpyDeviceToHost) == hipSuccess) {
            long long bad = 0;
            for (long long i = 0; i < done; ++i) bad += h[(size_t)i] != (unsigned long long)i + 1ull;
            if (bad) { set_error("dpr_launch_bench: " + std::to_string(bad) + " of " + std::to_string(done) + " replayed launches did not run with their own parameters"); rc_marks = DPR_ERR_STATE; }
        }
    }
    return rc_marks;
}

// measurement aid (round 4): a background load on a stream of its own -- `blocks` workgroups of 64 threads spin on FMAs until
// dpr_spin_stop sets the flag or `max_ms` of the 100 MHz wall clock have passed (every wave reaches that exit).  Used to find out
// whether the latency-bound loops run at reduced clocks when the chip is otherwise idle (profiles/nj_target.py --spin).
__global__ void dpr_spin_kernel(const unsigned int* flag, unsigned long long max_ticks, double* sink)
{
    const unsigned long long t0 = wall_clock64();
    double x = 1.0 + threadIdx.x * 1e-9, y = 0.999999;
    for (;;) {
#pragma unroll
        for (int k = 0; k < 256; ++k) x = x * y + 1e-12;
        if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) break;
        if (wall_clock64() - t0 > max_ticks) break;
    }
    if (x == 12345.678) *sink = x;
}
static hipStream_t g_spin_stream = nullptr;
static unsigned int* g_spin_flag = nullptr;      // host-pinned, device-visible
static double* g_spin_sink = nullptr;
int dpr_spin_start(dpr_ctx* c, int blocks, int max_ms)
{
    if (!c || blocks < 1 || blocks > 4096 || max_ms < 1 || max_ms > 60000) { set_error("dpr_spin_start: bad argument"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    if (!g_spin_stream) {
        int least = 0, greatest = 0;
        DPR_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        DPR_HIP(hipStreamCreateWithPriority(&g_spin_stream, hipStreamNonBlocking, least));
        DPR_HIP(hipHostMalloc(reinterpret_cast<void**>(&g_spin_flag), sizeof(unsigned int), hipHostMallocMapped));
        DPR_HIP(hipMalloc(&g_spin_sink, sizeof(double)));
    }
    *g_spin_flag = 0u;
    hipLaunchKernelGGL(dpr_spin_kernel, dim3((unsigned)blocks), dim3(64), 0, g_spin_stream, (const unsigned int*)g_spin_flag,
                       (unsigned long long)max_ms * 100000ull, g_spin_sink);
    DPR_HIP(hipGetLastError());
    return DPR_OK;
}
int dpr_spin_stop(dpr_ctx* c)
{
    if (!c || !g_spin_stream) { set_error("dpr_spin_stop: not started"); return DPR_ERR_STATE; }
    *g_spin_flag = 1u;
    DPR_HIP(hipStreamSynchronize(g_spin_stream));
    return DPR_OK;
}

// tuning hook: row-group size (16/32/64), non-temporal loads (0/1), scan grid (<= 2048; 0 = default)
int dpr_scan_tune(int rg, int nt, int grid)
{
    if (((rg & 127) != 16 && (rg & 127) != 64) || grid < 0 || grid > kScanBlocks) { set_error("dpr_scan_tune: bad argument"); return DPR_ERR_ARG; }
    nj_scan_config(rg, nt, grid);
    return DPR_OK;
}

// calibration: average ms of a plain streaming read of `bytes` of the matrix buffer
int dpr_bw_probe(dpr_ctx* c, int64_t bytes, int nt, int grid, int reps, float* out_ms)
{
    if (!c || !c->have_matrix || !out_ms || grid < 1 || reps < 1) { set_error("dpr_bw_probe: bad argument"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    // the buffer the Q-argmin scans: the position-space matrix of the pruned path (whose tip-order matrix is dead
    // once the first epoch is built), else this rank's rows
    NjBuffers& b = c->nj[0];
    const double* buf = b.pr.in_positions() ? b.pr.D : b.D;
    const int64_t cap = b.pr.in_positions() ? b.pr.P * b.pr.ld * (int64_t)sizeof(double) : b.rows_local * b.ld * (int64_t)sizeof(double);
    if (!buf || cap <= 0) { set_error("dpr_bw_probe: no matrix buffer"); return DPR_ERR_STATE; }
    return nj_bw_probe(buf, cap, b.xpart, bytes, nt, grid, reps, c->stream, c->ev[2], c->ev[3], out_ms);
}

// ---- test hooks ---------------------------------------------------------------------------------------------
int64_t dpr_n_active(dpr_ctx* c)
{
    if (!c || !c->have_matrix) { set_error("dpr_n_active: no matrix"); return DPR_ERR_STATE; }
    NjState st;
    if (int rc = fetch_state(c, &st)) return rc;
    return st.n;
}

int64_t dpr_n_total(dpr_ctx* c) { return c ? c->nj[0].N : DPR_ERR_ARG; }

int dpr_get_matrix_row(dpr_ctx* c, int64_t i, double* out)
{
    if (!c || !c->have_matrix || !out || i < 0 || i >= c->nj[0].N) { set_error("dpr_get_matrix_row: bad argument"); return DPR_ERR_ARG; }
    DPR_HIP(hipStreamSynchronize(c->stream));   // the plain copies below run on the null stream, which does not wait for c->stream
    const NjPruned& q = c->nj[0].pr;
    const int64_t N = c->nj[0].N;
    if (!q.in_positions()) {
        const double* src = slot_row(c, i, 0, false);
        if (!src) { set_error("dpr_get_matrix_row: row not owned by this rank"); return DPR_ERR_ARG; }
        DPR_HIP(hipMemcpy(out, src, sizeof(double) * (size_t)N, hipMemcpyDeviceToHost));
        return DPR_OK;
    }
    // position space: row of slot i, columns gathered through pos_of_slot (dead slots read +inf)
    std::vector<int32_t> pos((size_t)N);
    std::vector<double> row((size_t)q.P);
    DPR_HIP(hipMemcpy(pos.data(), q.pos_of_slot, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost));
    if (pos[(size_t)i] < 0 || pos[(size_t)i] >= q.P) {      // slot not alive any more
        for (int64_t j = 0; j < N; ++j) out[j] = __builtin_inf();
        return DPR_OK;
    }
    DPR_HIP(hipMemcpy(row.data(), slot_row(c, i, pos[(size_t)i], false), sizeof(double) * (size_t)q.P, hipMemcpyDeviceToHost));
    for (int64_t j = 0; j < N; ++j) out[j] = (pos[(size_t)j] >= 0 && pos[(size_t)j] < q.P) ? row[(size_t)pos[(size_t)j]] : __builtin_inf();
    return DPR_OK;
}

int dpr_get_row_sums(dpr_ctx* c, double* out)
{
    if (!c || !c->have_matrix || !out) { set_error("dpr_get_row_sums: bad argument"); return DPR_ERR_ARG; }
    DPR_HIP(hipStreamSynchronize(c->stream));   // the plain copies below run on the null stream, which does not wait for c->stream
    if (c->nj[0].pr.in_positions()) {
        NjPruned& q = c->nj[0].pr;
        const int64_t N = c->nj[0].N;
        std::vector<int32_t> pos((size_t)N);
        std::vector<double> u((size_t)q.P);
        NjState st;
        if (int rc = fetch_state(c, &st)) return rc;
        DPR_HIP(hipMemcpy(pos.data(), q.pos_of_slot, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToHost));
        DPR_HIP(hipMemcpy(u.data(), njp_current_u(q, st.it), sizeof(double) * (size_t)q.P, hipMemcpyDeviceToHost));
        for (int64_t j = 0; j < N; ++j) out[j] = (pos[(size_t)j] >= 0 && pos[(size_t)j] < q.P) ? u[(size_t)pos[(size_t)j]] : 0.0;
        return DPR_OK;
    }
    DPR_HIP(hipMemcpy(out, c->nj[0].U, sizeof(double) * (size_t)c->nj[0].N, hipMemcpyDeviceToHost));
    return DPR_OK;
}

int dpr_get_msa_counts(dpr_ctx* c, int64_t row, int32_t* useful, int32_t* match)
{
    if (!c || !c->msa.planes || row < 0 || row >= c->msa.n) { set_error("dpr_get_msa_counts: bad argument"); return DPR_ERR_ARG; }
    if (row == 0) return DPR_OK;
    DevBuf<int32_t> du, dm;
    DPR_HIP(du.alloc((size_t)row));
    DPR_HIP(dm.alloc((size_t)row));
    if (int rc = msa_counts_row(c->msa, row, du, dm, c->stream)) return rc;
    DPR_HIP(hipStreamSynchronize(c->stream));
    DPR_HIP(hipMemcpy(useful, du, sizeof(int32_t) * (size_t)row, hipMemcpyDeviceToHost));
    DPR_HIP(hipMemcpy(match, dm, sizeof(int32_t) * (size_t)row, hipMemcpyDeviceToHost));
    return DPR_OK;
}

// test / measurement hook: the distance block of tips [row0, row0 + nrows) against tips [0, ncols) through the launcher the
// placement batches, --add and the divide-and-conquer assignment use (msa_dist_block_rows; MSADistConstructionRangeDC of
// src/divide_and_conquer/msa.cu:321-372 computes the same block a row at a time).  out (optional, host): row-major
// [nrows][ncols], or [ncols][nrows] when transposed; reps >= 1 launches, *ms_avg their average duration (HIP events).
int dpr_msa_dist_block(dpr_ctx* c, int64_t row0, int64_t nrows, int64_t ncols, int dist_type, int transposed, double* out, int reps, float* ms_avg)
{
    if (!c || !c->msa.planes || row0 < 0 || nrows < 1 || row0 + nrows > c->msa.n || ncols < 1 || ncols > c->msa.n || reps < 1) { set_error("dpr_msa_dist_block: bad argument"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    DevBuf<double> d;
    const int64_t ld = transposed ? nrows : ncols;
    DPR_HIP(d.alloc((size_t)(nrows * ncols)));
    int rc = msa_dist_block_rows(c->msa, row0, nrows, 0, 0, ncols, dist_type, d, ld, c->stream, transposed != 0);      // warm
    ScopedEvent e0, e1;
    if (rc == DPR_OK && (hipEventCreate(e0.put()) != hipSuccess || hipEventCreate(e1.put()) != hipSuccess)) rc = DPR_ERR_HIP;
    if (rc == DPR_OK) {
        (void)hipEventRecord(e0, c->stream);
        for (int r = 0; r < reps && rc == DPR_OK; ++r) rc = msa_dist_block_rows(c->msa, row0, nrows, 0, 0, ncols, dist_type, d, ld, c->stream, transposed != 0);
        (void)hipEventRecord(e1, c->stream);
    }
    if (rc == DPR_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = DPR_ERR_HIP;
    float ms = 0;
    if (rc == DPR_OK) (void)hipEventElapsedTime(&ms, e0, e1);
    if (ms_avg) *ms_avg = ms / (float)reps;
    if (rc == DPR_OK && out && hipMemcpy(out, d, sizeof(double) * (size_t)(nrows * ncols), hipMemcpyDeviceToHost) != hipSuccess) rc = DPR_ERR_HIP;
    if (rc == DPR_ERR_HIP) { (void)hipGetLastError(); set_error("dpr_msa_dist_block: HIP error"); }
    return rc;
}

int dpr_get_timing(dpr_ctx* c, double* dist_ms, double* nj_ms)
{
    if (!c) { set_error("dpr_get_timing: null ctx"); return DPR_ERR_ARG; }
    if (dist_ms) *dist_ms = c->dist_ms;
    if (nj_ms) *nj_ms = c->nj_ms;
    return DPR_OK;
}

}  // extern "C"
