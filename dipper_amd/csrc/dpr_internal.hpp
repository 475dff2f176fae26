// Internal declarations shared by the HIP translation units of libdipper_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "../../include/dipper_hip.h"
#include "hip_scope.hpp"

namespace dpr {

constexpr int kRowBlock = DPR_ROW_BLOCK;  // rows per ownership block == rows per scan tile
constexpr int kTileCols = 512;            // columns per scan tile (256 lanes x 2 doubles)
constexpr int kScanBlocks = 8192;         // capacity of the partials array (scan grid <= this)
constexpr int kThreads = 256;

void set_error(const std::string& msg);
// stderr logging of the library, ONE variable: DPR_LOG = comma list of categories, optionally with a level: epoch[=1|2|3]
// (pruned NJ: epoch rebuilds and graph captures; 2: + units listed per watched window; 3: + laps of a rebuild), mash (kernel
// choice, index sizes), import (backbone import rounds), cli (start-up and phase laps of the `dipper` command).  0 = off.
int log_level(const char* category);
int hip_fail(hipError_t e, const char* what);
#define DPR_HIP(call)                                            \
    do {                                                         \
        hipError_t e__ = (call);                                 \
        if (e__ != hipSuccess) return dpr::hip_fail(e__, #call); \
    } while (0)

// ---- sharding (block-cyclic by kRowBlock rows) -------------------------------------------------
__host__ __device__ inline int shard_owner(int64_t row, int world)
{
    return (int)((row / kRowBlock) % world);
}
__host__ __device__ inline int64_t shard_local_row(int64_t row, int world)
{
    return (row / kRowBlock / world) * kRowBlock + row % kRowBlock;
}
__host__ __device__ inline int64_t shard_global_row(int64_t local, int rank, int world)
{
    return ((local / kRowBlock) * world + rank) * kRowBlock + local % kRowBlock;
}
__host__ __device__ inline int64_t shard_rows(int64_t n, int rank, int world)
{
    // number of slots < n owned by rank
    int64_t nblk = n / kRowBlock, rem = n % kRowBlock;
    int64_t full = nblk / world + ((nblk % world) > rank ? 1 : 0);
    int64_t cnt = full * kRowBlock;
    if (rem && (nblk % world) == rank) cnt += rem;
    return cnt;
}

// ---- tie-break key of the reference's findMinDist + thrust::min_element -------------------------
// (src/neighborJoining.cu:124-146,214): preference (band(i), j mod 256, j, i).
__host__ __device__ inline uint64_t nj_band(int64_t i, int64_t n)
{
    int64_t sz0 = n / 256, rem = n % 256, thr = (sz0 + 1) * rem;
    return (uint64_t)(i < thr ? i / (sz0 + 1) : rem + (i - thr) / sz0);
}
__host__ __device__ inline uint64_t nj_key_a(int64_t i, int64_t n)  // part depending on "i"
{
    return (nj_band(i, n) << 56) | (uint64_t)i;
}
__host__ __device__ inline uint64_t nj_key_b(int64_t j)  // part depending on "j"
{
    return ((uint64_t)(j & 255) << 48) | ((uint64_t)j << 24);
}

// ---- bootstrap column sample (boot.hip; dpr_msa_boot_weights restates it on the host from the same functions) -------------
// splitmix64's finaliser.  Replicate r of an alignment of L sites (L < 2^32) draws column_t = ((mix64(key_r ^ t) >> 32) * L) >> 32,
// t = 0 .. L-1, key_r = mix64(seed ^ mix64(r)); uint64 arithmetic, wrapping.
__host__ __device__ inline uint64_t mix64(uint64_t z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__host__ __device__ inline uint64_t boot_key(uint64_t seed, int64_t replicate) { return mix64(seed ^ mix64((uint64_t)replicate)); }
__host__ __device__ inline int64_t boot_column(uint64_t key, int64_t t, int64_t L)
{
    return (int64_t)(((mix64(key ^ (uint64_t)t) >> 32) * (uint64_t)L) >> 32);
}

struct alignas(32) NjRecord {
    double q;
    uint64_t key;
    double d;
    uint64_t pad;
};

struct NjState {
    int64_t n;       // active size
    int64_t it;      // iterations done
    int32_t x, y;    // slots merged in the current iteration (x<y)
    double d;        // D[x][y]
    double q;        // winning Q value
    int32_t status;  // 0 ok, 1 = no candidate (DPR_ERR_NOCAND)
    int32_t pad;     // njs.hip: 1 once a failed rank has announced its status to the other ranks (it does so once)
    // pruned path (graph-replayed kernels read their iteration from memory): `it` is advanced by the post kernel while
    // it runs, so the post kernel reads `itb`, which the scan kernel (that reads `it`) publishes for it
    int64_t itb;
    int64_t it_limit;  // iterations >= it_limit are no-ops
    int64_t N;         // tips
    unsigned long long cnt_list[4];   // units listed for the scan of iteration it: cnt_list[it % 3]
    unsigned long long units_scanned; // statistics
    // pnew[it & 1]: position of the node created by merge it-1 (-1: none).  During iteration it that node is in
    // QUARANTINE: its row sum is not materialised yet (Ur = NaN, so the unit scans skip it), its pairs are evaluated
    // by the scan kernel's new-row blocks from the row buffer R[(it - 1) & 1]
    int32_t pnew[2];
};

// position-space state of the pruned path (njp.hip)
struct NjPruned {
    bool active = false;
    int64_t P = 0, ld = 0;      // positions of this epoch, row stride
    double* D = nullptr;        // [P][ld] position space
    double* U = nullptr;        // [2][vstride] by position, double-buffered: iteration it reads U + (it & 1) * vstride
    double* Ur = nullptr;       // by position; NaN for dead positions and for the node in quarantine
    double* R = nullptr;        // [2][vstride] row of the node created by merge it: R + (it & 1) * vstride
    int64_t vstride = 0;
    uint64_t *KA = nullptr, *KB = nullptr;  // key parts from the reference slot of each position
    // njp_post2_kernel (large shape): header + arrays its producer blocks hand to its test blocks (in the epoch's slab)
    bool range_known = false;         // t2_hdr holds the range of every entry of this run (njp_range_kernel + the M parts since)
    char* t2_hdr = nullptr; double *t2_rmax = nullptr, *t2_cmax = nullptr, *t2_colmin = nullptr, *t2_rowmin = nullptr, *t2_cmin = nullptr;
    int32_t *slot_of_pos = nullptr, *pos_of_slot = nullptr, *perm = nullptr;   // slot_of_pos < 0: dead position
    uint64_t* umin = nullptr;   // [strips][groups][4][2] order-encoded lower bound of D per sub-unit and row half (readers take the smaller word)
    int64_t nunits_alloc = 0, utot = 0;
    int64_t utot0 = 0;          // units of one full scan at the first epoch (statistics)
    bool fresh = false;         // epoch just built: the first scan is a full one (njp_list_all_kernel), nothing in quarantine
    // unit-sharded mode (several GPUs, each holding the whole position-space matrix): unit ownership by
    // (strip * G16 + group) % sh_world; sh_virtual: all ranks are emulated in this process (validation)
    int sh_world = 1, sh_rank = 0;
    bool sh_virtual = false;
    int (*gather)(void* ctx, void* buf, size_t bytes_per_rank, hipStream_t s) = nullptr;   // in-place all-gather of the block records
    void* gather_ctx = nullptr;
    unsigned long long* cnt_all = nullptr;   // [local ranks][4] list counters (index it % 3)
    int64_t list_stride = 0;
    // Arena, kept until nj_free (a context that builds a matrix of the same size again allocates nothing):
    // one matrix buffer of the pruned path's own -- the epochs alternate between it and NjBuffers::D, whose tip-order
    // contents are dead once epoch 0 is built -- and two slabs for the per-epoch vectors (an epoch rebuild reads the
    // old epoch's vectors while it writes the new one's).
    double* arena_D = nullptr;
    char* arena_slab[2] = { nullptr, nullptr };
    size_t arena_slab_bytes = 0;
    int64_t arena_N = 0;
    int arena_ranks = 0;
    int epoch_index = 0;             // epoch e uses slab e & 1; its matrix lives in arena_D for even e, in NjBuffers::D for odd e
    hipGraphExec_t graph = nullptr;   // graph_iters iterations of (scan, post)
    // plan of THIS context (set by njp_build; two contexts of one process may differ and run on different host threads)
    int scan_grid = 512;              // blocks of the unit scan (DPR_NJP_GRID)
    int graph_iters = 32;             // iterations per captured hipGraph (DPR_NJ_GRAPH_ITERS)
    // Adaptive plan (single rank): the exact pruned scan only pays while its bounds prune.  The host looks at the units
    // listed per iteration after the first graph of an epoch and then every 2 048 iterations; once more than stream_frac of
    // the epoch's units are listed on average, the run is HANDED OVER to the streaming loop of nj.hip: the live positions
    // are permuted back into a dense slot-space matrix (one n^2 copy) and the reference's own algorithm -- one full Q scan
    // per iteration, last slot moved into y -- continues from the same state (same keys, same update arithmetic, so the
    // same merge log).  Every so often (after the active size has shrunk by the epoch factor once, twice, four times, ...
    // while the probes keep failing) a fresh pruned epoch is built from the slot-space matrix and probed again.
    int adaptive = 1;                 // DPR_NJ_ADAPTIVE=0 / dpr_ctx_set_nj_adaptive
    double stream_frac = 0.7;         // DPR_NJ_STREAM_FRAC (tests force the hand-over with 0); a listed unit costs ~1.6 x a streamed one, part of its sub-units are skipped
    bool slots_mode = false;          // the run currently lives in slot space (b.D, b.U, b.Ur, b.KA: nj.hip's loop)
    int64_t slots_probe_n = 0;        // slots mode: build and probe a pruned epoch again once the active size is <= this
    int probe_fail_streak = 0;
    int64_t stream_iterations = 0, stream_epochs = 0;     // iterations run by the streaming loop / hand-overs, since the matrix was built
    bool in_positions() const { return active && !slots_mode; }     // the matrix and the vectors of the moment are the position-space ones
    unsigned long long* dbg = nullptr;   // DPR_NJ_PHASES: [2 kernels][2048 blocks][8 stamps], then 32768 words of accumulate-mode statistics
    int64_t dbg_it = -1;
    int32_t* list = nullptr;         // units selected by the tests (sub-unit mask << 28 | strip << 18 | group)
    int32_t *blk_cb = nullptr, *blk_g0 = nullptr;   // test block -> (strip, first group)
    int nprep = 0;
};

// optional per-kernel timing of the pruned NJ loop (dpr_ctx_set_nj_kernel_timing): the run is enqueued eagerly and every
// stride-th iteration's launches are bracketed by HIP events on the library's stream
constexpr int kNjKernelsMax = 6;
struct NjKernelTiming {
    int stride = 0;                    // 0 = off
    int nk = 0;                        // kernels per iteration of the last timed run
    std::vector<hipEvent_t> ev;        // (nk + 1) events per sampled iteration
    double us_sum[kNjKernelsMax] = { 0, 0, 0, 0, 0, 0 };
    int64_t samples = 0;
};
// one more event of a sampled iteration, recorded on s (on = false: nothing)
inline int nj_timing_mark(NjKernelTiming* kt, bool on, hipStream_t s)
{
    if (!on) return DPR_OK;
    hipEvent_t e = nullptr;
    DPR_HIP(hipEventCreate(&e));
    kt->ev.push_back(e);
    DPR_HIP(hipEventRecord(e, s));
    return DPR_OK;
}

// ---- one-exchange row-sharded streaming NJ (njs.hip) --------------------------------------------------------------
constexpr int kNjsMaxWorld = 64;
constexpr unsigned int kNjsTicketGroups = 32;                                   // two-level last-block ticket of njs_scan_kernel
constexpr size_t kNjsTicketBytes = 128 * (1 + (size_t)kNjsTicketGroups);       // one 128-byte line per counter
constexpr int kNjsLegacy = 0;    // round 2's loop: 4 launches + 2 all-gathers per iteration (nj.hip)
constexpr int kNjsPeer = 1;      // 2 launches + ONE RCCL all-gather (rank records); rows x / y pulled from their owners' memory
constexpr int kNjsMailbox = 2;   // 2 launches, no collective: the records go straight into every rank's mailbox
// A rank's record of one iteration as the one-exchange loop publishes it (one 64-byte line).  Besides the rank's best
// candidate it carries what lets every rank CHECK the others each iteration (round 4; the loop has no fences and had
// never met a second GPU):
//   seq     run id << 32 | it + 1 -- written last; a record of another iteration means the exchange did not happen;
//   ux      bits of the row sum U[x] of the node created by merge it - 1 as THIS rank computed it: a sum over values
//           derived from every element of the rows x and y the rank pulled from their owners.  The row sums are
//           replicated state, bit-identical on every rank by construction, so one differing word proves that some rank
//           pulled stale or torn data -- the run ends with DPR_ERR_COMM instead of a silently different merge log;
//   status  the publishing rank's state (3 / 4: it has already failed) -- the others fail the same way, not with NOCAND.
struct alignas(64) NjsRec {
    double q;
    uint64_t key;
    double d;
    uint64_t seq;
    uint64_t ux;
    uint64_t status;
    uint64_t pad[2];
};
// layout of a rank's peer-visible window (byte offsets): mail[2][kNjsMaxWorld] records (NjsRec) | barrier lines | slice | 4 row buffers
struct NjsLayout {
    int64_t off_bar = 0, off_slice = 0, off_rows = 0, bytes = 0;
    int64_t off_njr = 0;     // region of the row-sharded pruned NJ (njr.hip), 0 = none
    int64_t slice_len = 0;   // doubles (initial row sums of the own rows)
    int64_t ldv = 0;         // doubles per row buffer
};
struct NjPeer {
    int plan = kNjsLegacy;
    char* win = nullptr;             // this rank's window (fine-grained device memory)
    NjsLayout lay;
    unsigned int* ticket = nullptr;  // last-block tickets of the scan (kNjsTicketBytes)
    char** d_win = nullptr;          // device arrays [kNjsMaxWorld]: every rank's window / matrix as mapped into THIS process
    double** d_D = nullptr;
    std::vector<double*> h_D;        // host copy of d_D
    std::vector<char*> h_win;        // host copy of d_win
    std::vector<void*> opened;       // hipIpc mappings to close
    bool attached = false;
    unsigned long long bar_epoch = 0;
    unsigned long long run_id = 0;   // matrix builds on this window so far (part of every mail sequence number)
    unsigned long long poll_ticks = 200000000ull;    // 2 s of the 100 MHz wall clock
    int64_t fault_it = -1; int fault_rank = -1;      // test hook (dpr_ctx_set_debug_fault)
};

// ---- row-sharded pruned NJ (njr.hip): the position-space matrix of njp.hip with its rows dealt to the ranks ------------
// Chunk k of kNjrChunk positions (64 row groups: the rows of one test block of njp_post_kernel<64, 1>) belongs to rank
// k % world; a rank stores its chunks one behind the other at full width.  Units, their bounds, lists and scans belong to
// the owner of their rows.
constexpr int kNjrChunk = 1024;
constexpr int kNjrCollective = 1;        // block records and column slices travel by all-gathers (RCCL; device copies between virtual ranks)
constexpr int kNjrMailbox = 2;           // ... by stores straight into every rank's window: no collective
__host__ __device__ inline int njr_owner(int64_t p, int world) { return (int)((p / kNjrChunk) % world); }
__host__ __device__ inline int64_t njr_local_row(int64_t p, int world) { return (p / kNjrChunk / world) * kNjrChunk + p % kNjrChunk; }
__host__ __device__ inline int64_t njr_global_pos(int64_t l, int rank, int world) { return ((l / kNjrChunk) * world + rank) * kNjrChunk + l % kNjrChunk; }
// matrix rows a rank must be able to hold for P positions (whole chunks)
__host__ __device__ inline int64_t njr_rows_cap(int64_t P, int world)
{
    const int64_t chunks = (P + kNjrChunk - 1) / kNjrChunk;
    return ((chunks + world - 1) / world) * kNjrChunk;
}
// doubles per exchanged column slice: local rows of positions < N + 2 chunks (the kernels read vectors up to 511 positions
// behind P and an even index behind the last position)
__host__ __device__ inline int64_t njr_slice_len(int64_t N, int world) { return ((N / kNjrChunk + 2 + world - 1) / world) * kNjrChunk; }
// the njr region of a rank's peer-visible window (offsets relative to the region's start)
struct NjrLayout {
    int64_t off_recflag = 0, off_recs = 0, off_rowflag = 0, off_rows = 0, bytes = 0;
    int64_t rec_stride = 0;     // records per (parity, source rank): unit-scan blocks per rank + 1 header record
    int64_t slice = 0;          // doubles per column slice
};
struct NjRowShard {
    int world = 1, rank = 0, plan = 0;     // world > 1: active
    NjrLayout lay;
    int64_t win_off = 0;                   // start of the njr region inside the window (NjPeer::win)
    double* rows_plain = nullptr;          // collective plan: [world][2][slice] all-gather buffer (mailbox plan: the window's region)
    double* stage = nullptr;               // epoch builds: source rows pulled from their owners, [stage_rows][stage_ld]
    int64_t stage_rows = 0, stage_ld = 0;
    char** d_region = nullptr;             // device array [world]: the njr regions of all ranks' windows
    double** d_src = nullptr;              // device array [world]: source buffers of the epoch build in progress
    unsigned int* ticket = nullptr;        // last-block tickets of SCAN and EXTRACT (2 x kNjsTicketBytes)
    double* half[2] = { nullptr, nullptr };   // the two epoch buffers of this rank (halves of NjBuffers::D)
    std::vector<double*> peer_half[2];     // ... of every rank, as mapped into this process (epoch builds pull from them)
    int (*gather)(void* ctx, int kind, hipStream_t s) = nullptr;   // collective plan: kind 0 = block records (in place, b.partials), 1 = column slices (in place, rows_plain)
    int (*barrier)(void* ctx) = nullptr;   // all ranks' streams idle and in step (epoch builds)
    void* cb_ctx = nullptr;
    int64_t launches = 0, collectives = 0;
};

struct NjBuffers {
    NjPeer peer;
    NjKernelTiming* kt = nullptr;   // owned by the context
    double* D = nullptr;       // [rows_local_max][ld] (+ tail pad)
    // row-sharded pruned NJ: D is ONE allocation of two halves of twin_rows rows each (the epochs of njr.hip alternate between
    // them; one hipIpc handle covers both); D points at the first half, which also receives the tip-order rows
    int64_t twin_rows = 0;
    size_t half_bytes = 0;
    int64_t ld = 0;
    int64_t N = 0;             // total tips
    int64_t rows_local = 0;    // local rows at n = N
    double* U = nullptr;       // [N] replicated
    double* Ur = nullptr;      // [N] U/(n-2) for the current n
    uint64_t* KA = nullptr;    // [N] nj_key_a(i, n) for the current n
    NjRecord* partials = nullptr;  // [kScanBlocks]
    NjRecord* recs = nullptr;      // [world]
    NjsRec* recs64 = nullptr;      // [world] rank records of the one-exchange loop (njs.hip)
    double* xpart = nullptr;   // [ceil(N/256)]
    double* gath = nullptr;    // [3][world][slice] gathered column slices (world > 1)
    double* slice = nullptr;   // [3][slice] local column slices (world > 1)
    int64_t slice_len = 0;
    NjState* st = nullptr;
    int32_t* log_x = nullptr;  // [N]
    int32_t* log_y = nullptr;
    double* log_bx = nullptr;
    double* log_by = nullptr;
    // BIONJ (dpr_ctx_set_nj_variant(ctx, 1); nullptr while the context builds NJ trees)
    double* V = nullptr;       // variances: layout and row stride of D, a copy of D (pads included) once the distance source has filled it
    double* vpart = nullptr;   // [ceil(N/256)] chunk partials of the lambda sum of the current iteration
    double* bj = nullptr;      // [4] unclamped bx0, by0 and vxy = V[y][x] of the current iteration (nj_bionj_lambda_kernel -> nj_bionj_post_kernel)
    double* log_lam = nullptr; // [N] lambda of every iteration, beside the merge log
    int rank = 0, world = 1;
    NjPruned pr;
    NjRowShard rs;
};

// nj.hip
int nj_alloc(NjBuffers& b, int64_t N, int rank, int world, hipStream_t s, int64_t twin_rows = 0, bool bionj = false);   // fills ordered on s; same shape again: buffers kept (bionj: + V and its vectors; without: they are released)
int nj_bionj_init(NjBuffers& b, hipStream_t s);                                      // V = D (the whole buffer), once the distance source has filled D
int nj_launch_bionj_lambda(NjBuffers& b, int64_t n, hipStream_t s);                  // chunk partials of the lambda sum, bx0 / by0 / vxy
int nj_launch_bionj_post(NjBuffers& b, int64_t n, int64_t it, hipStream_t s);        // select + commit + weighted update of D, V, U
int nj_fill_pads(double* D, int64_t ld, int64_t nrows, int64_t ncols, int64_t rows_alloc, int64_t tail, bool diag, hipStream_t s);
void nj_free(NjBuffers& b);
int nj_expand_lower(NjBuffers& b, const double* d_packed_lower, hipStream_t s);
int nj_init_sums(NjBuffers& b, hipStream_t s, double* local_sums = nullptr);   // U (one rank) or the own rows' sums, state
int nj_prepare(NjBuffers& b, hipStream_t s);            // Ur, KA for n = st->n
int nj_launch_scan(NjBuffers& b, bool probe, int64_t n, int64_t it, hipStream_t s);
void nj_scan_config(int rg, int nt, int grid);  // tuning knobs (dpr_scan_tune)
int nj_scan_grid();
int nj_bw_probe(const double* buf, int64_t cap_bytes, double* sink, int64_t bytes, int nt, int grid, int reps, hipStream_t s, hipEvent_t e0,
                hipEvent_t e1, float* ms);
int nj_launch_post(NjBuffers& b, int64_t n, int64_t it, hipStream_t s);            // world == 1
int nj_launch_select_local(NjBuffers& b, int nparts, hipStream_t s);                            // -> b.recs[b.rank]
int nj_launch_commit_extract(NjBuffers& b, int64_t n, int64_t it, hipStream_t s);   // world > 1
int nj_launch_update_sharded(NjBuffers& b, int64_t n, hipStream_t s);               // world > 1
int nj_launch_unpack_u(NjBuffers& b, hipStream_t s);                                // world > 1: gathered row sums -> U
int nj_launch_finish(NjBuffers& b, int64_t n, int64_t it, hipStream_t s);           // materialise U[x] after the loop

// njs.hip: one-exchange row-sharded loop (world > 1)
NjsLayout njs_layout(int64_t N, int world, bool with_njr = false);
int njs_alloc_window(NjBuffers& b, hipStream_t s);
void njs_free_window(NjBuffers& b);
int njs_set_peers(NjBuffers& b, char* const* wins, double* const* Ds, hipStream_t s);
int njs_launch_scan(NjBuffers& b, int64_t n, int64_t it, bool pending, hipStream_t s);
int njs_launch_post(NjBuffers& b, int64_t n, int64_t it, bool pending, hipStream_t s);
int njs_launch_finish(NjBuffers& b, int64_t n, int64_t it, bool pending, hipStream_t s);
int njs_launch_barrier(NjBuffers& b, hipStream_t s);
int njs_launch_unpack_u(NjBuffers& b, hipStream_t s);

// njr.hip: row-sharded exact pruned NJ (world > 1; NjRowShard)
NjrLayout njr_layout(int64_t N, int world);
int njr_build(std::vector<NjBuffers*>& ranks, hipStream_t s);      // the ranks held by this process (all of them: virtual ranks; one: a process rank)
int njr_run(std::vector<NjBuffers*>& ranks, int64_t it0, int64_t todo, hipStream_t s);
void njr_free(NjBuffers& b);

// njp.hip: exact pruned NJ (world == 1)
int njp_build(NjBuffers& b, hipStream_t s);   // permute the tip-order matrix by ascending row sum into the pruned path's own buffer
void njp_free(NjPruned& q);                   // everything, the arena included
int njp_arena(NjPruned& q, int64_t N, hipStream_t s);     // allocate the arena for N tips (njp_build; ahead of it: dpr_reserve_nj)
void njp_reset(NjPruned& q);                  // epoch state only (graph, pointers); the arena stays for the next build
int njp_unit_owner(int64_t strip, int64_t group, int64_t P, int world);
int njp_run(NjBuffers& b, int64_t it0, int64_t todo, hipStream_t s);   // enqueue `todo` iterations (hipGraph replays)
const char* njp_kernel_name(int idx);   // intervals of one timed iteration of the LAST timed run, in launch order
void njp_set_kernel_names(const char* const* names);     // (up to kNjKernelsMax, "" terminated; names in () are not kernels)
int njp_phase_stamps(unsigned long long* out);   // debug (DPR_NJ_PHASES)
int njp_debug_list(NjBuffers& b, int32_t* out, int64_t cap, int64_t* count, int64_t* P, double* ur, int64_t urcap);   // debug
const double* njp_current_u(const NjPruned& q, int64_t it);
int njp_shape(const NjPruned& q, int64_t* positions, int* row_groups, int* strips, int* post2, int* scan_grid);   // launch shape of the current epoch   // row sums by position after `it` iterations

// Divide-and-conquer cluster distances (dc.hip builds the jobs; msa.hip / mash.hip run them).
// Cluster ci has cl_m[ci] members (tip ids members[cl_moff[ci] + t], ascending) and a leaf list
// cols[cl_coff[ci] + u], u < kDcLeaves + m: the 2 x 5 closest leaves of the cluster edge and of its
// reverse (-1 = empty list entry), then the members.  Element (t, u), u < kDcLeaves + t, of its
// distance block is out[cl_out[ci] + t * cl_ld[ci] + u] = distance(row tip members[t], column tip cols[u]).
constexpr int kDcLeaves = 10;
struct PairJobs {
    const int4* jobs;          // (cluster, first row t0, first column u0, -)
    const int32_t* members;
    const int32_t* cols;
    const int64_t* cl_moff;
    const int32_t* cl_m;
    const int64_t* cl_coff;
    const int64_t* cl_out;
    const int32_t* cl_ld;
    double* out;
};

// msa.hip
struct MsaBuffers {
    uint32_t* planes = nullptr;  // [4][n][W32]: X (not a base), LO, HI, LX = LO | X bit planes, 32 bases per word
    int64_t n = 0, L = 0, W32 = 0;
    // alignments of at most kMsaTabSites sites: the distance of every (useful, match) pair of counts, types 1 and 2 -- the same
    // function of the same two integers as the epilogue computes, read instead of recomputed (a division and a log per pair are
    // half of the pair kernel's instructions at 400 sites)
    double* jc_tab = nullptr;    // [2][(L + 1) * (L + 1)]; longer alignments: the band [2][kMsaBand + 1][L + 1] (useful = L - g)
    // per sequence: bit j = its 16-word stage j holds a not-a-base position (gap, N, padding); stages from 63 on share bit 63
    unsigned long long* xstage = nullptr;
    // bootstrap replicates (boot.hip): planes / xstage above are the ACTIVE alignment's; alt_* is the other set -- the
    // replicate buffers while the uploaded alignment is active, the uploaded alignment's while a replicate is (a replicate
    // has the same L, so jc_tab serves both)
    uint32_t* alt_planes = nullptr;
    unsigned long long* alt_xstage = nullptr;
    int32_t* boot_w = nullptr;      // [L] multiplicity of every column in the active replicate
    uint32_t* boot_incl = nullptr;  // [L] inclusive scan of boot_w
    int32_t* boot_src = nullptr;    // [32 W32] source column of every replicate position, -1 = padding
    int64_t replicate = -1;         // active replicate, -1 = the uploaded alignment
    // protein alignment (msa_aa.hip): planes is then [6][n][W32] -- X (not a residue), then the five bits of code + 1, all 0 where
    // X -- xstage as above, aa_nx[n] the not-a-residue positions of every sequence among its 32 W32; no jc_tab, no replicates
    bool aa = false;
    int32_t* aa_nx = nullptr;
};
constexpr int64_t kMsaTabSites = 1024;
constexpr int kMsaBand = 15;
int msa_upload(MsaBuffers& m, const uint64_t* packed4, int64_t n, int64_t L, hipStream_t s);
void msa_free(MsaBuffers& m);
int msa_restage(MsaBuffers& m, hipStream_t s);     // m.xstage of the active planes again (nothing to do without xstage)
// everything that follows from the planes alone (jc_tab, xstage): allocated for m.n / m.L, then filled from m.planes
int msa_derived_alloc(MsaBuffers& m);
int msa_derive(MsaBuffers& m, hipStream_t s);
// mash_index.hip: out[i] = in[0] + ... + in[i] (in and out must not alias); synchronises s
int mi_inclusive_scan(const uint32_t* in, uint32_t* out, int64_t n, hipStream_t s);
int msa_dist_rows(const MsaBuffers& m, NjBuffers& b, int dist_type, hipStream_t s);
int msa_dist_tile_edge(const MsaBuffers& m, int dist_type);   // rows/columns per job tile of msa_dist_jobs
int msa_counts_row(const MsaBuffers& m, int64_t row, int32_t* d_useful, int32_t* d_match, hipStream_t s);

// ---- transfer bootstrap expectation (tbe.hip) ----------------------------------------------------------------------------
// The main tree is uploaded when its merge log differs from the last one (host copy kept): once per command.
struct TbeBuffers {
    int64_t n = 0, cap = 0;              // tips of the uploaded main tree; tips the buffers hold
    std::vector<int32_t> hx, hy;         // the uploaded main merge log
    std::vector<int32_t> mpos;           // main-order rank of every leaf
    std::vector<int32_t> node;           // k of every listed main node (internal node n+k with min(|A|, n-|A|) >= 2)
    std::vector<int32_t> size;           // |A| of every listed main node
    std::vector<int32_t> hphi;           // phi of the listed nodes, copied back
    int2* main_iv = nullptr;             // [listed] main clade as [S, E) in the main tree's DFS leaf order
    int32_t* m = nullptr;                // [n] main-order rank of the leaf at every replicate DFS position
    int2* rep_iv = nullptr;              // [n-2] replicate internal node n+k as [s, e) in the replicate's DFS leaf order
    int32_t* phi = nullptr;              // [listed]
    uint4* scratch = nullptr;            // tables of the global-memory variant (none until a tree needs it)
    size_t scratch_bytes = 0;
    // dpr_transfer_taxa only (none of it is allocated before its first call)
    int32_t skip = -1;                   // listed index of the root child left out of the branches (both root children listed), or -1
    int64_t taxa_cap = 0;                // tips phi_arg and moved hold
    int32_t* phi_arg = nullptr;          // [2 listed] phi, then the closest replicate node: 2 x its place in rep_iv + (h > n - h)
    int32_t* moved = nullptr;            // [n] by replicate DFS position: counted branches of this call whose transfer set holds the tip
    std::vector<int32_t> hmoved;         // moved, copied back
};
void tbe_free(TbeBuffers& t);

// ---- balanced minimum evolution NNI (bme.hip) ------------------------------------------------------------------------------------
// Kept by the context from the first dpr_bme_nni on (a later call over no more tips allocates nothing); released with it.
struct BmeBuffers {
    DevBuf<double> T;                    // [M][ld] table of subtree averages over the M = 2n - 2 nodes (S and W, see bme_host.hpp), by place in rank order
    DevBuf<int32_t> itab;                // [9][ldi]: kid0, kid1, par, sib, height, tin, tout, rows, pos (place of a node in T)
    DevBuf<double> out;                  // [2][ldi]: length of the edge above every node, gain
    DevBuf<int32_t> omove;               // [ldi] candidate move of every node (0: none)
    int64_t cap_n = 0, ld = 0, ldi = 0;  // tips the buffers hold, row stride of T, stride of the small arrays
    int64_t allocations = 0;             // device allocations made for this context so far
    int64_t launches = 0, evaluations = 0;       // kernels / table builds of the last call
    double table_ms = 0, select_ms = 0;  // of the last call: table (fill, S, W) / lengths + gains and their copy back (HIP events)
    // dpr_bme_spr only (none of it is allocated before its first call)
    DevBuf<int32_t> spr_tab;             // [5][spr_ldi]: per place of T the record kid0, kid1, par, clade size (places), then the node id of every place
    DevBuf<double> spr_gain;             // [9][spr_ldi]: best gain per (directed subtree, side) (4), per directed subtree (2); three averages per place (3)
    DevBuf<int32_t> spr_wk;              // [12][spr_ldi]: target w and path length k per (subtree, side) (4 + 4), per subtree (2 + 2)
    DevBuf<double> spr_dstack;           // traversal stacks of the scan, one column per resident thread: U, V, h ...
    DevBuf<int32_t> spr_istack;          // ... and node, node before it, k
    int64_t spr_ldi = 0;                 // stride the three arrays above were sized for
    int64_t spr_allocations = 0;         // device allocations dpr_bme_spr has made for this context beyond the table's
    int64_t spr_launches = 0;            // scan kernels of the last dpr_bme_spr
    double spr_scan_ms = 0;              // of the last dpr_bme_spr: mirror, scan, best and their copy back (HIP events)
};

// ---- UPGMA / WPGMA (upgma.hip) ---------------------------------------------------------------------------------------------------
// Kept by the context from the first dpr_upgma_run on (a later call over no more tips allocates nothing); released with it.
struct UpgmaBuffers {
    DevBuf<double> D;                    // [cap_n][ld] working copy of the matrix, both triangles
    DevBuf<double> size;                 // [cap_n] tips under every active slot
    DevBuf<uint64_t> nkey;               // [cap_n] nearest neighbour of every active row: key of its distance ...
    DevBuf<int32_t> nn;                  // ... and its slot
    DevBuf<int32_t> list;                // [cap_n] rows to scan again this iteration
    DevBuf<int32_t> log_x, log_y;        // [cap_n] the merge log
    DevBuf<double> log_h;                // [cap_n] height of every merge
    DevBuf<char> st;                     // the loop's state (UpgmaState)
    int64_t cap_n = 0, ld = 0;           // tips the buffers hold, row stride of D
    int64_t allocations = 0;             // device allocations made for this context so far
    int64_t launches = 0, rescanned = 0; // of the last call: kernels, rows scanned again
    double loop_ms = 0;                  // of the last call: the n - 1 iterations (HIP events)
};

// ---- fit of a tree to the matrix (fit.hip) ---------------------------------------------------------------------------------------
// Kept by the context from the first dpr_tree_fit / dpr_tree_patristic_rows on (a later call over no more tips allocates nothing).
struct FitBuffers {
    DevBuf<int32_t> rank;                // [cap_n] place of every tip in the depth-first order
    DevBuf<double> dtip;                 // [cap_n] depth of every tip
    DevBuf<double> dnode;                // [cap_n] depth of the internal nodes by order index
    DevBuf<int32_t> tab;                 // [levels][n - 1] sparse table of order indices (cap_levels * cap_n entries held)
    DevBuf<double> dpart;                // [9][cap_n]: the seven row parts, the row maxima, the column parts of e e; then scratch row sums
    DevBuf<int32_t> ipart;               // [5][cap_n]: three row counts, the maxima's j, the column counts
    int64_t cap_n = 0, cap_levels = 0;
    int64_t allocations = 0;             // device allocations made for this context so far
    int64_t launches = 0, levels = 0;    // of the last dpr_tree_fit: kernels, rows of its table
    double row_ms = 0, col_ms = 0, rowsum_ms = 0;      // of the last dpr_tree_fit (HIP events)
    int compare = 0;                     // dpr_ctx_set_fit_compare: time the NJ row-sum kernel beside the passes
};

// ---- pairs within a threshold and their components (pairs.hip; driver in ctx_pairs.hip) --------------------------------------------
// Everything lives from dpr_pairs_begin to dpr_pairs_end (or the next begin, or dpr_destroy); nothing of the context's other state is
// touched.  Device memory: the row block, the pair buffers (grown to the largest block met, at most block_rows * n entries), O(n) for
// the parents and O(block_rows) for the counts.
using PinnedBuf = HipOwner<void*, hipHostFree>;
constexpr int kPairsThreads = 256;                       // one workgroup walks one row
constexpr int kPairsChunk = 2 * kPairsThreads;           // columns per step of the walk: two per lane, kPairsThreads apart
constexpr int64_t kPairsBlockBytes = (int64_t)1 << 30;   // block_rows 0: the row block takes at most this much
constexpr int64_t kPairsMaxRows = 32768;                 // rows of one block, whatever was asked for (the whole matrix is built in such blocks too)
struct PairsBuffers {
    bool ended = false, labelled = false;
    int source = 0, dist_type = 0;
    double threshold = 0;
    int64_t n = 0, block_rows = 0, ld = 0, next_row = 0;
    DevBuf<double> block;                // [block_rows][ld] rows of the current block (MSA, Mash; the packed triangle is read in place)
    DevBuf<int64_t> cnt;                 // [block_rows + 1] pairs kept per row, then their exclusive scan in place; [nr] the block's total
    DevBuf<int32_t> pi, pj;              // [cap] the block's pairs, ordered
    DevBuf<double> pd;
    DevBuf<int32_t> parent;              // [n] union-find forest: parent[v] <= v
    int64_t cap = 0;
    PinnedBuf hi, hj, hd, htotal;        // host side of pi / pj / pd (cap entries each) and of the block's total
    int64_t dev_bytes = 0, peak_bytes = 0;
    int64_t blocks = 0, pairs = 0, comps = 0, largest = 0, singletons = 0;
    double dist_ms = 0, filter_ms = 0, copy_ms = 0;      // summed over the blocks (HIP events): the provider; count + scan + write + hook; the copies back
};
// rows [r0, r0 + nr): row i's entries j < i are rows[(i - r0) * ld + j], or -- packed -- rows[i (i - 1) / 2 + j] (rows = the triangle)
int pairs_count_scan(const double* rows, int64_t ld, bool packed, int64_t r0, int64_t nr, double threshold, int64_t* cnt, hipStream_t s);   // cnt[t] = first pair of row r0 + t, cnt[nr] = total
int pairs_write_hook(const double* rows, int64_t ld, bool packed, int64_t r0, int64_t nr, double threshold, const int64_t* cnt, int64_t total,
                     int32_t* pi, int32_t* pj, double* pd, int32_t* parent, int64_t n, hipStream_t s);
int pairs_parent_init(int32_t* parent, int64_t n, hipStream_t s);
int pairs_flatten(const int32_t* parent, int32_t* out, int64_t n, hipStream_t s);      // out[v] = root of v (out may be parent itself)
int pairs_hook(const int32_t* pi, const int32_t* pj, int64_t total, int32_t* parent, int64_t n, hipStream_t s);      // the union of `total` pairs into the forest (device arrays)

// ---- each sequence's K nearest neighbours (nearest.hip; driver in ctx_nearest.hip) ---------------------------------------------------
// Everything lives from dpr_nearest_begin to dpr_nearest_end (or the next begin, or dpr_destroy), beside and independent of a stream of
// pairs.  Device memory: one block of full rows (every source: the packed triangle is expanded into it) and block_rows * K results.
constexpr int kNearestMaxK = 256;                        // 1 <= K <= kNearestMaxK
constexpr int kNearestThreads = 256;                     // one workgroup walks one row
constexpr int kNearestChunk = 4 * kNearestThreads;       // columns per step of the walk: two 16-byte loads per lane
constexpr int kNearestCap = kNearestChunk + 2 * kNearestMaxK;      // candidates held in LDS: a step always fits behind a selection's K
struct NearestBuffers {
    int source = 0, dist_type = 0, K = 0;
    int64_t n = 0, block_rows = 0, ld = 0, next_row = 0;
    DevBuf<double> block;                // [block_rows][ld] full rows of the current block
    DevBuf<int32_t> oj, ocnt, oflush;    // [block_rows][K] columns; [block_rows] real entries; [block_rows] selections a row needed before its last
    DevBuf<double> od;                   // [block_rows][K] distances
    PinnedBuf hj, hd, hcnt, hflush;      // host side of the four
    int64_t dev_bytes = 0, peak_bytes = 0;
    int64_t blocks = 0, neighbours = 0, fewer = 0, none = 0, flushes = 0;
    double dist_ms = 0, select_ms = 0, copy_ms = 0;      // summed over the blocks (HIP events): the provider (or the expansion); the select; the copies back
};
// the sortable key of a distance: the bits of d (of +0.0 for either zero) with the sign bit flipped for d >= 0 and all bits flipped for
// d < 0 -- unsigned order of the keys = fp64 order of the finite distances (nearest.hip, mst.hip)
__device__ inline unsigned long long nearest_key(double d)
{
    unsigned long long b = d == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(d);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ inline bool nearest_finite(double d)
{
    return ((unsigned long long)__double_as_longlong(d) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}
// rows [r0, r0 + nr) of the packed triangle as full rows: out[(i - r0) * ld + j] = D_ij for j < n (0 on the diagonal)
int nearest_expand_packed(const double* lower, int64_t n, int64_t r0, int64_t nr, double* out, int64_t ld, hipStream_t s);
// row r0 + t = rows[t * ld + 0 .. n): its K nearest into oj / od [t * K ..], ocnt[t], oflush[t]
int nearest_select(const double* rows, int64_t ld, int64_t r0, int64_t nr, int64_t n, int K, int32_t* oj, double* od, int32_t* ocnt,
                   int32_t* oflush, hipStream_t s);

// ---- the minimum spanning forest of the distances (mst.hip; driver in ctx_mst.hip) -------------------------------------------------------
// Boruvka rounds over streamed blocks of full rows.  What a call allocates lives for the call; the context keeps the figures of the last
// one (dpr_mst_stats, dpr_get_mst_info).
constexpr int kMstThreads = 256;                         // one workgroup walks one row
constexpr int kMstChunk = 4 * kMstThreads;               // columns per step of the walk: two 16-byte loads per lane
struct MstState {
    int64_t n = 0, block_rows = 0;
    int64_t rounds = 0, blocks = 0, edges = 0, comps = 0, largest = 0, singletons = 0, peak_bytes = 0, rows_walked = 0;
    double dist_ms = 0, rowmin_ms = 0, round_ms = 0;      // summed over the rounds (HIP events): the provider (or the expansion); the row minimum; the component work and the copies
};
// row r0 + t = rows[t * ld + 0 .. n): the smallest (key, c) over the columns c < n with label[c] != label[r0 + t] and a finite entry
// into rkey / rcol / rdist [r0 + t] (rdist: that entry's own bits); an all-ones key, column -1 for none.  label: ld entries readable.
int mst_row_min(const double* rows, int64_t ld, int64_t r0, int64_t nr, int64_t n, const int32_t* label, unsigned long long* rkey,
                int32_t* rcol, double* rdist, hipStream_t s);
// per component (named by its root, label[v] == v) the smallest (key, max(r, c), min(r, c)) of its rows into ckey / cedge, both all-ones
// before; then every root with an edge appends it behind *count in ei / ej / ed (cap places) unless the component at the other end
// chose the same edge and has the smaller label
int mst_component_min_emit(const int32_t* label, const unsigned long long* rkey, const int32_t* rcol, const double* rdist, int64_t n,
                           unsigned long long* ckey, unsigned long long* cedge, int32_t* ei, int32_t* ej, double* ed, int64_t cap,
                           unsigned long long* count, hipStream_t s);

// mash.hip
// inverted index over the sketches (mash_index.hip): per chunk of kIC = 1 024 tips the (value -> tips, positions) postings
struct MashIndex {
    uint32_t* post = nullptr;    // [n*S] per chunk sorted by value: 2 * (tip mod kIC) << 16 | position; tip kIC - 1 + position 65535 = not a first copy
    uint64_t* uniq = nullptr;    // [nu] distinct values, chunk after chunk
    uint32_t* off = nullptr;     // [nu + 1] first posting of each distinct value
    uint32_t* bkt = nullptr;     // [chunks][65537] directory on the leading bits: first distinct value of each bucket
    uint32_t* ubase = nullptr;   // [chunks + 1] first distinct value of each chunk
    int32_t* shift = nullptr;    // [chunks] bucket = value >> shift
    uint64_t* vmax = nullptr;    // [chunks] largest value
    uint16_t* mult = nullptr;    // [n*S] copies of the value at its first position in a sketch, 0 elsewhere
    double* dtab = nullptr;      // [S + 1] distance of every count
    int32_t* dblk = nullptr;     // [nu] dense block of the value or -1
    uint16_t* dense = nullptr;   // [ndense][kIC] position of the value in every tip of the chunk, 0x7F7F = absent (+ 64 entries of padding)
    int64_t chunks = 0;
    uint32_t nu = 0, ndense = 0;
};

struct MashBuffers {
    uint64_t* packed2 = nullptr;   // flat 2-bit packed reads
    uint64_t* word_off = nullptr;  // [n]
    uint64_t* len = nullptr;       // [n] bases
    uint64_t* sketches = nullptr;  // [n][S] ascending
    // run encoding of every sketch against ONE reference list (mash_encode, see mash.hip): tokens [n][S] of 16 bytes,
    // tok_cnt[n]; ref = the reference's distinct values (ref_n of them)
    uint4* tokens = nullptr;
    int32_t* tok_cnt = nullptr;
    uint64_t* ref = nullptr;
    int ref_n = 0;
    double tok_mean = 0.0;         // tokens per sketch (sampled): the token kernel is used while this stays small
    MashIndex index;               // built when the sketches do not resemble each other (or DPR_MASH_INDEX=1)
    bool share_chip = false;       // the next distance launches run beside tree kernels of another stream: leave wave slots free
    uint64_t total_words = 0;
    int64_t n = 0;
    int S = 0, k = 0;
};
int mash_upload(MashBuffers& m, const uint64_t* packed2, const uint64_t* word_off, const uint64_t* len,
                int64_t n, hipStream_t s);
void mash_free(MashBuffers& m);
int mash_sketch(MashBuffers& m, int k, int S, hipStream_t s);
// rows r0..r0+nr (world > 0: owned local rows of (rank,world); world == 0: plain tip ids) x columns
// [0,ncols) -> out[t*ld + j]; full = also j >= i
int mash_dist_rows(const MashBuffers& m, int64_t r0, int64_t nr, int rank, int world, bool full,
                   int64_t ncols, double* out, int64_t ld, hipStream_t s, bool transposed = false);
int mash_dist_jobs(const MashBuffers& m, const PairJobs& J, int njobs, hipStream_t s);
// mash_index.hip
int mash_index_build(MashBuffers& m, hipStream_t s);
void mash_index_free(MashIndex& ix);
// built, kIC, chunks, nu, ndense, kIDenseMin, largest sketch size, tasks of a launch beside tree kernels above which its grid is bounded
void mash_index_info(const MashIndex& ix, int64_t info[8]);
int mash_dist_index(const MashBuffers& m, int64_t r0, int64_t nr, int64_t ncols, double* out, int64_t ld, double* mir,
                    bool transposed, hipStream_t s, int rank, int world);
// the whole Mash matrix of a rank whose rows are sharded by row blocks (world > 1): D_local holds its rows at full width
int mash_dist_matrix_sharded(const MashBuffers& m, int rank, int world, int64_t rows_local, double* D_local, int64_t ld, hipStream_t s);
int mash_jobs_rows();   // members per job
int mash_jobs_cols();   // leaf-list positions per job
int mash_hash_positions(const MashBuffers& m, int64_t seq, int k, uint64_t* d_out, uint64_t len, uint64_t word_off,
                        hipStream_t s);

// What a block of the pair kernels computes: up to PT row sequences x PT column sequences (ids in LDS, -1 = none) and
// where the PT x PT tile of distances goes.
constexpr int64_t kNoDiag = (int64_t)1 << 40;
struct MsaSparseX { const unsigned long long* stage; };
struct TileOut {
    double* out;        // element (r, c) of the tile -> out[r * ld + c]            (row-major target)
    int64_t ld;
    int nr, nc;         // valid rows / columns of the tile
    int lower_base;     // >= 0: keep only c_pos < lower_base + r_pos (tile-local positions + tile origins below)
    int r_org, c_org;   // positions of the tile origin inside its job (for lower_base)
    double* mir;        // != nullptr: also element (r, c) -> mir[c * mir_ld + r]  (mirror / transposed target)
    int64_t mir_ld;
    bool skip_main;     // only the transposed target is written
    int64_t diag;       // element (r, c) with r + diag == c is a tip against itself -> 0 (kNoDiag: none)
    const double* tab;  // types 1-2: distance by (useful, match): tab_ld > 0 the full table of a short alignment (row stride tab_ld),
    int tab_ld;         // tab_ld < 0 the band useful >= L - kMsaBand of a long one (L = -tab_ld - 1); nullptr: computed
    const unsigned long long* xstage;   // types 1-2: per sequence, the stages that hold a not-a-base position (nullptr: every stage of every sequence)
};
// msa_aa.hip: the protein alphabet behind the same entry points (msa.hip dispatches on MsaBuffers::aa)
int msa_aa_upload(MsaBuffers& m, const uint8_t* codes, int64_t n, int64_t L, hipStream_t s);
int msa_aa_derived_alloc(MsaBuffers& m);      // xstage, aa_nx
int msa_aa_derive(MsaBuffers& m, hipStream_t s);
int msa_aa_launch(int dist_type, hipStream_t s, const MsaBuffers& m, double* D, int64_t ld, int64_t rows, int rank, int world,
                  int64_t row0, int64_t col0, int64_t ncols, int transposed);
int msa_aa_counts_row(const MsaBuffers& m, int64_t row, int32_t* d_useful, int32_t* d_match, hipStream_t s);

// msa.hip: same row-provider shape as mash_dist_rows
// transposed: out[j * ld + t] instead of out[t * ld + j]
int msa_dist_block_rows(const MsaBuffers& m, int64_t r0, int64_t nr, int rank, int world, int64_t ncols,
                        int dist_type, double* out, int64_t ld, hipStream_t s, bool transposed = false);
int msa_dist_jobs(const MsaBuffers& m, int dist_type, const PairJobs& J, int njobs, hipStream_t s);

// place.hip
struct PlaceBuffers {
    int64_t N = 0;   // tips the arrays are sized for; internal node ids start at N
    int64_t M = 0;   // tips of the edge scan's slot range (4M-4 slots): N, or the backbone size in DC mode
    int32_t *head = nullptr, *e = nullptr, *nxt = nullptr, *belong = nullptr, *rev = nullptr, *cid = nullptr;
    int32_t* cont = nullptr;     // [16N] per slot u->v: the (up to two) slots leaving v other than v->u (-1 none; -2: v has degree > 3, walk its list)
    double *len = nullptr, *cdis = nullptr;
    int32_t *q_id = nullptr, *q_from = nullptr;
    double* q_dis = nullptr;
    void* partials = nullptr;
    int nparts_max = 0;
    void* partials_multi = nullptr;   // block minima of a scan launch that serves several tips (place_tips)
    int64_t nparts_multi = 0;
    int dbg = 0;   // 4: place_update_kernel writes its phase clocks into the trace (DPR_PLACE_CLOCKS, profiling only)
    // Edge records (round 5): a read-optimised MIRROR of what the per-tip scan (calculateBranchLength, src/placement_close_k.cu:
    // 309-358) needs, one entry per UNDIRECTED edge = the slot pair s / rev[s]; side 0 is the slot with belong >= e (the one the
    // reference evaluates), side 1 its reverse.  Struct of arrays (every load of the scan coalesced); the slot-indexed arrays
    // above stay the authoritative state -- the split and the closest-list BFS write both.
    double* er_d = nullptr;      // [11][ecap]: cdis of side 0 (fields 0..4), of side 1 (5..9), len (10)
    int32_t* er_i = nullptr;     // [12][ecap]: cid of side 0 (0..4), of side 1 (5..9), slot of side 0 (10), slot of side 1 (11)
    int32_t* eidx = nullptr;     // [8N] slot -> 2 * edge + side
    int64_t ecap = 0;
    int32_t* bfs_cnt = nullptr;  // [N] per placed tip: slots its closest-list walk reached beyond the two rounds the split applies (negative: -(n + 1), the walk of a node of degree > 3)
    int32_t* misc = nullptr;     // [0]: smallest live slot with belong < e (its tuple (0, 0, 2) competes for the first minimum); [1]: edge counter of an import
};
int place_alloc(PlaceBuffers& p, int64_t N, int64_t M = 0);   // M = 0: M = N
void place_free(PlaceBuffers& p);
int place_init_fresh(PlaceBuffers& p, hipStream_t s);
int place_initial_tree(PlaceBuffers& p, const double* d_dis_row1, hipStream_t s);
int place_import_backbone(PlaceBuffers& p, int64_t m, hipStream_t s);
int place_tip(PlaceBuffers& p, const double* d_dis, int64_t tip, double* d_trace, hipStream_t s);
int place_tips(PlaceBuffers& p, const double* d_dis0, int64_t ldb, int64_t tip0, int64_t count, double* d_trace, hipStream_t s);
int64_t place_multi_min();        // first tip of the four-tip launch pairs

// exact.hip: exact placement mode (src/placement.cu)
struct XStep {                   // counters of the two node lists, status words (device)
    int nroot[2], ntop[2];       // [parity of the rank buffers the lists belong to]: px_patch_kernel of tip i fills [(i + 1) & 1] and clears [i & 1]
    int poll_fail, poll_node, poll_pass;   // px_top_poll: a value never arrived (node on record, pass 0 bottom-up / 1 top-down): the run fails
    int quirk;                   // the reference's swap in updateTreeStructure was taken: its depths are no tree depths any more (see exact.hip)
};
struct ExactBuffers {
    double* lim = nullptr;       // [8N] per directed slot
    int32_t* dep = nullptr;      // [2N] depth below node N
    int32_t* rk[2] = { nullptr, nullptr };   // [2N] DFS pre-order rank, double-buffered: placing tip i reads rk[i & 1] and writes rk[(i + 1) & 1]
    int32_t* sz[2] = { nullptr, nullptr };   // [2N] nodes in the subtree, same buffering
    int32_t* nar = nullptr;      // [2N] node at rank
    int32_t* tix = nullptr;      // [2N] top node -> index in the level-sorted top list (-1: not a top node)
    int32_t* roots = nullptr;    // [2N] x int4: roots of the small subtrees (<= sm nodes, parent's subtree larger): node, rank, size, depth
    int32_t* tops = nullptr;     // nodes whose subtree has more than 64 nodes
    int32_t* order = nullptr;    // [2N] top nodes grouped by depth
    int32_t* lvoff = nullptr;    // [2N+2] first index of every level in order[]
    int32_t* hist = nullptr;     // [2N+2]
    int32_t* nd = nullptr;       // [2N][12] node records: slot[3], reverse slot[3], target node[3], pad
    XStep* st = nullptr;
    void* tpack = nullptr;       // [kTopClimb] structural records of the top nodes, packed beside the small-subtree pass (px_top_climb)
    void* partials = nullptr;
    int32_t* dfsrk = nullptr;    // literal schedule: the reference's single rank array (alias of rk[0])
    bool literal = false;        // run the literal one-workgroup schedule (fallback / DPR_EXACT_LITERAL=1)
    unsigned long long* clk = nullptr;   // DPR_EXACT_CLOCKS=1 (profiling): phase clocks of px_top_kernel, summed over the tips (100 MHz ticks)
    int sm = 64;                 // nodes of a small subtree for the next patch launch (64 / 256 / 1 024: exact_adapt)
    int sm_forced = 0;           // tests (DPR_EXACT_SM=64|256|1024): no adaptation
    int pass_sm = 64;            // ... of the passes that are enqueued last (their workgroups' partials are what the next patch reads)
    bool top_poll = false;       // tests / A-B (DPR_EXACT_TOP_POLL=1): the polling schedule of px_top_poll even where the climbing one applies
    bool top_levels = false;     // tests / A-B (DPR_EXACT_TOP_LEVELS=1): the top-tree pass level by level with a workgroup barrier per level (rounds 3-5)
    bool top_in_memory = false;  // tests (DPR_EXACT_TOP_MEM=1): the top-tree pass keeps its values in memory even when they fit LDS
};
int exact_alloc(ExactBuffers& x, int64_t N);
void exact_free(ExactBuffers& x);
int exact_init(PlaceBuffers& p, ExactBuffers& x, const double* d_dis_row1, const double* d_dis_row2, bool has_tip2,
               hipStream_t s);
int exact_tip(PlaceBuffers& p, ExactBuffers& x, int64_t tip, const double* d_dis_next, bool has_next, double* d_trace,
              hipStream_t s);
int exact_adapt(ExactBuffers& x, hipStream_t s);                 // between batches of tips: larger small subtrees when the top tree approaches its LDS capacity
int exact_quirk(ExactBuffers& x, hipStream_t s, bool* quirk);    // did the fast schedule meet the case only the literal one reproduces?

// dc.hip: divide-and-conquer mode (cluster assignment + concurrent cluster trees)
struct DcTable {
    int nv = 0;                    // eligible backbone slots (belong >= e), ascending
    int32_t* vslots = nullptr;
    int32_t* et_cid = nullptr;     // [nv][10] closest ids: own list, reverse list
    double* et_cdis = nullptr;     // [nv][10]
    double* et_len = nullptr;      // [nv]
    // chunks of consecutive table entries (tree order) whose closest lists name at most kDcRows distinct backbone tips: the assignment
    // scan stages those tips' distance rows in LDS once per (chunk, 64 queries)
    int nch = 0;
    int32_t* ch_e0 = nullptr;      // [nch + 1] first table entry of a chunk
    int32_t* ch_l0 = nullptr;      // [nch + 1] first entry of a chunk in ch_leaf
    int32_t* ch_leaf = nullptr;    // the chunks' distinct backbone tips
    int max_entries = 0, max_leaves = 0;      // most table entries / most distinct tips in one chunk (dpr_get_dc_table_stats)
    uint4* et_rec = nullptr;       // [nv][11] x 16 B per entry: for each of the 10 list entries {LDS offset (in doubles) of its staged row (absent: the
                                   // -inf row), 0, path length}; then {slot, 0, edge length} -- copied to LDS per chunk, read there at a wave-uniform address
    double* part_add = nullptr;    // [chunks][ldq] per-chunk first minima
    int32_t* part_pos = nullptr;
    size_t part_cap = 0;
};
struct DcStats { int64_t clusters = 0, max_cluster = 0, pairs = 0, groups = 0, jobs = 0; };
int dc_table_build(PlaceBuffers& p, int64_t B, DcTable& t, hipStream_t s);
void dc_table_free(DcTable& t);
// dT[c * ldq + q] = distance(query q of the batch, backbone tip c); d_cluster_id[q] = chosen slot
int dc_assign(DcTable& t, const double* dT, int64_t ldq, int Q, int32_t* d_cluster_id, hipStream_t s);
int dc_parts_reserve(DcTable& t, int64_t ldq);     // part_add / part_pos for a scan of ldq query columns
int dc_cluster_phase(PlaceBuffers& p, const int32_t* h_cluster_id, int64_t N, int64_t B, int source, int dist_type,
                     const MsaBuffers* msa, const MashBuffers* mash, double* d_trace, size_t budget_bytes,
                     DcStats* stats, int rank, int world, hipStream_t s);
// multi-rank merge of the cluster phase: every array element is changed by at most one rank, so
// new = old + sum over ranks of (new - old) in wrap-around integer arithmetic (doubles as their bit patterns)
void dc_deal_clusters(const int64_t* sizes_desc, int64_t count, int world, int32_t* owner);
void dc_query_share(int64_t n, int64_t B, int rank, int world, int64_t* q0, int64_t* q1);
int dc_delta_sub(void* cur, const void* old, int64_t words64, hipStream_t s);   // cur -= old (64-bit words)
int dc_delta_add(void* cur, const void* old, int64_t words64, hipStream_t s);   // cur += old

// pfix.hip: independent placement of queries on a FIXED backbone (no reference counterpart).  The backbone's edge table (the
// divide-and-conquer assignment's DcTable: dense records, LDS-sized chunks) is built once by dpr_place_fixed_set and kept; every
// dpr_place_fixed_run scores all (query, eligible slot) pairs with the arithmetic of calculateBranchLength and returns, per
// query, the eligible slot with the smallest (pendant length, slot), the position on it and the pendant length.
struct PlaceFixed {
    bool valid = false;            // the table belongs to the backbone of the last dpr_place_fixed_set
    int64_t m = 0, n = 0;          // backbone tips, all tips
    int64_t batch = 0;             // test hook (dpr_ctx_set_place_fixed_batch): queries per batch, 0 = the rule of dpr_dc_run
    DcTable tab;
    int32_t* ent_of_slot = nullptr;    // [4m - 4] table entry of an eligible slot, -1 elsewhere
    double* part_frac = nullptr;       // [chunks][ldq] positions of the per-chunk minima (the carrying scan only)
    size_t part_frac_cap = 0;
    double* dT = nullptr;              // [m][Q] query-minor distance block of a batch
    size_t dT_cap = 0;
    int32_t* slot = nullptr;           // [share x ranks] results of the last run
    double *frac = nullptr, *add = nullptr;
    size_t out_cap = 0;
};
int pfix_set(PlaceFixed& f, PlaceBuffers& p, int64_t m, hipStream_t s);       // p holds the imported backbone and its lists
void pfix_free(PlaceFixed& f);
// dT[c * ldq + q] = distance(query q of the batch, backbone tip c); slot / frac / add[q] of the Q queries.  carry: the scan carries
// the position through its loop instead of the reduce step evaluating the winning entry again (same bits either way)
int pfix_place(PlaceFixed& f, const double* dT, int64_t ldq, int Q, int32_t* d_slot, double* d_frac, double* d_add, bool carry,
               hipStream_t s);

}  // namespace dpr
