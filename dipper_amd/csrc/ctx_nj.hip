// C ABI, distance matrix and neighbor joining: plan selection (dpr_nj_plan_resolve: the only place that chooses among the seven
// DPR_NJ_PLAN_* kinds), dpr_dist_matrix, dpr_nj_run, dpr_argmin_once and the NJ getters.
// BIONJ (dpr_ctx_set_nj_variant): always the streaming loop on the rank's own copy; dpr_nj_variant_host restates that loop on the host.
#include "ctx_internal.hpp"

#include <chrono>
#include <cstdio>

namespace dpr {
// NJ algorithm on a single GPU: 1 = exact pruned scan (njp.hip, default), 0 = full streaming scan
static int g_nj_mode = -1;
static int g_nj_vshards = 1;   // > 1: a single-rank context emulates that many unit-sharded ranks (validation)
// Several ranks, pruned NJ: 0 = auto (unit-sharded scans from kNjShardTips tips on, below that every rank runs the
// single-GPU plan on its own copy: an iteration is then ~20 us of dependent latency and a collective per iteration
// would only add to it; ROW-SHARDED pruned -- njr.hip -- once two copies of the matrix no longer fit one GPU), 1 = always
// unit-sharded, 2 = never, 3 = row-sharded pruned (dpr_set_nj_multi_plan / DPR_NJ_MULTI=auto|shard|solo|rows)
static int g_nj_multi_plan = -1;
constexpr int64_t kNjShardTips = 65536;
static int nj_multi_plan()
{
    if (g_nj_multi_plan < 0) {
        const char* e = std::getenv("DPR_NJ_MULTI");
        g_nj_multi_plan = (e && std::strcmp(e, "shard") == 0) ? 1 : (e && std::strcmp(e, "solo") == 0) ? 2 : (e && std::strcmp(e, "rows") == 0) ? 3 : 0;
    }
    return g_nj_multi_plan;
}

bool want_pruned(const dpr_ctx* c)
{
    if (c->nj_mode >= 0) return c->nj_mode == 1;
    if (g_nj_mode < 0) {
        const char* e = std::getenv("DPR_NJ_MODE");
        g_nj_mode = (e && std::strcmp(e, "stream") == 0) ? 0 : 1;
    }
    return g_nj_mode == 1;
}
static int g_nj_exchange = -1;
int ctx_exchange_plan(const dpr_ctx* c)
{
    if (c->local_comm) return kNjsMailbox;
    if (c->nj_exchange >= 0) return c->nj_exchange;
    if (g_nj_exchange < 0) {
        const char* e = std::getenv("DPR_NJ_EXCHANGE");
        // Default LEGACY (round 4, advisor): the one-exchange plans have only ever run with virtual ranks and process ranks on
        // ONE device, where peer memory is local; until `bench.py --gpus G` has shown `matches_single_gpu` for them on real
        // multi-GPU hardware they are opt-in (DPR_NJ_EXCHANGE=peer|mailbox, dpr_ctx_set_nj_exchange -- bench.py times all three).
        g_nj_exchange = (e && std::strcmp(e, "peer") == 0) ? kNjsPeer : (e && std::strcmp(e, "mailbox") == 0) ? kNjsMailbox : kNjsLegacy;
    }
    return g_nj_exchange;
}
int ctx_multi_plan(const dpr_ctx* c) { return c->nj_multi_plan >= 0 ? c->nj_multi_plan : nj_multi_plan(); }
int ctx_vshards(const dpr_ctx* c) { return c->nj_vshards >= 1 ? c->nj_vshards : g_nj_vshards; }

// The plan this context sets up for n tips: its knobs as they stand now, and the device's memory where the resolver can ask for it
// (the auto rule of real ranks).  kind, or the resolver's error with the caller's name in front
int ctx_nj_plan(dpr_ctx* c, int64_t n, const char* who)
{
    size_t free_b = 0, total_b = 0;
    if (c->world > 1 && c->vworld == 0 && hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); total_b = ~(size_t)0; }   // (unknown: never too small)
    const int kind = dpr_nj_plan_resolve(c->world, c->vworld > 0, c->nj_variant, want_pruned(c), ctx_multi_plan(c), ctx_vshards(c), n, total_b);
    if (kind < 0) set_error(std::string(who) + ": " + last_error());
    return kind;
}
// matrix rows per epoch buffer of a rank under the rows-pruned plan: the same on every rank (the peers compute each other's second half)
int64_t njr_twin_rows(int64_t n, int world)
{
    const int64_t nblk = (n + kRowBlock - 1) / kRowBlock;
    const int64_t tip_rows = ((nblk + world - 1) / world) * kRowBlock + 32, pos_rows = njr_rows_cap(n, world);
    return tip_rows > pos_rows ? tip_rows : pos_rows;
}
static std::vector<NjBuffers*> njr_ranks(dpr_ctx* c)
{
    std::vector<NjBuffers*> v;
    for (auto& b : c->nj) v.push_back(&b);
    return v;
}
// Where the matrix row of slot `slot` can be read from this process (position space: `pos` is the slot's position, and the row's
// columns are positions); nullptr: another real rank holds it and no mapping of it exists here.  peer_matrix: the row may be read
// through the mapping of a peer's slot-space matrix -- for a caller that knows the peers' flushes are behind a barrier.
const double* slot_row(dpr_ctx* c, int64_t slot, int64_t pos, bool peer_matrix)
{
    NjBuffers& b0 = c->nj[0];
    const NjPruned& q = b0.pr;
    if (q.in_positions()) {
        if (c->plan.kind != DPR_NJ_PLAN_ROWS_PRUNED) return q.D + pos * q.ld;
        // rows dealt by position: the owner's epoch buffer of the moment, as mapped here
        return b0.rs.peer_half[(q.epoch_index + 1) & 1][(size_t)njr_owner(pos, c->world)] + njr_local_row(pos, c->world) * q.ld;
    }
    if (c->plan.whole_matrix()) return b0.D + slot * b0.ld;
    const int o = shard_owner(slot, c->world);
    const int64_t off = shard_local_row(slot, c->world) * b0.ld;
    if (c->vworld > 0) return c->nj[(size_t)o].D + off;
    if (o == c->rank) return b0.D + off;
    return peer_matrix && c->plan.exchange != kNjsLegacy && !b0.peer.h_D.empty() ? b0.peer.h_D[(size_t)o] + off : nullptr;
}
// one NJ iteration (active size n, iteration index it) of the eager streaming loops, on every rank held by this context
static int nj_iteration(dpr_ctx* c, int64_t n, int64_t it)
{
    NjBuffers& b0 = c->nj[0];
    switch (c->plan.kind) {
    case DPR_NJ_PLAN_BIONJ:
        // this rank's own copy whatever the world; the lambda kernel reads the rows of V that the update rewrites
        if (int rc = nj_launch_scan(b0, false, n, it, c->stream)) return rc;
        if (int rc = nj_launch_bionj_lambda(b0, n, c->stream)) return rc;
        c->nj_launches += 3;
        return nj_launch_bionj_post(b0, n, it, c->stream);
    case DPR_NJ_PLAN_SINGLE_STREAM:
        if (int rc = nj_launch_scan(b0, false, n, it, c->stream)) return rc;
        return nj_launch_post(b0, n, it, c->stream);
    case DPR_NJ_PLAN_ROWS_STREAM:
        break;
    default:
        set_error("dpr_nj_run: internal: the pruned plans have loops of their own");
        return DPR_ERR_STATE;
    }
    if (c->plan.one_exchange_loop()) {
        // one exchange, two launches (njs.hip): scan + record, [all-gather of the records | nothing: mailboxes], update
        for (auto& b : c->nj)
            if (int rc = njs_launch_scan(b, n, it, c->njs_pending, c->stream)) return rc;
        if (c->plan.exchange == kNjsPeer)
            if (int rc = exchange(c, EX_RECS64)) return rc;
        for (auto& b : c->nj)
            if (int rc = njs_launch_post(b, n, it, c->njs_pending, c->stream)) return rc;
        c->njs_pending = true;
        c->nj_launches += 2;
        return DPR_OK;
    }
    c->nj_launches += 4;
    for (auto& b : c->nj) {
        if (int rc = nj_launch_scan(b, false, n, it, c->stream)) return rc;
        if (int rc = nj_launch_select_local(b, nj_scan_grid(), c->stream)) return rc;
    }
    if (int rc = exchange(c, EX_RECS)) return rc;
    for (auto& b : c->nj)
        if (int rc = nj_launch_commit_extract(b, n, it, c->stream)) return rc;
    if (int rc = exchange(c, EX_SLICES)) return rc;
    for (auto& b : c->nj)
        if (int rc = nj_launch_update_sharded(b, n, c->stream)) return rc;
    return DPR_OK;
}

// ---- the steps of dpr_dist_matrix behind the source check and the resolver; each reads c->plan ------------------------------------
// the buffers of every rank held here; dealt rows also get their exchange set up (windows, peer mappings)
static int dist_alloc(dpr_ctx* c, int64_t n)
{
    // a whole copy (7.2 GB at 30 000 tips, 80 GB at 100 000) is allocated as rank 0 of 1, whatever the world
    const bool whole = c->plan.whole_matrix(), njr = c->plan.kind == DPR_NJ_PLAN_ROWS_PRUNED;
    for (size_t r = 0; r < c->nj.size(); ++r)
        if (int rc = nj_alloc(c->nj[r], n, whole ? 0 : (c->vworld > 0 ? (int)r : c->rank), whole ? 1 : c->world, c->stream, njr ? njr_twin_rows(n, c->world) : 0,
                              c->plan.kind == DPR_NJ_PLAN_BIONJ)) return rc;
    if (!c->plan.rows_dealt()) return DPR_OK;
    if (int rc = njs_setup(c, njr)) return rc;
    if (njr && c->plan.exchange == kNjsLegacy) {
        set_error("dpr_dist_matrix: the row-sharded pruned NJ needs the peers' buffers mapped on every rank (" + c->nj_exchange_note + "); use DPR_NJ_MODE=stream");
        return DPR_ERR_STATE;
    }
    return DPR_OK;
}
static int dist_fill(dpr_ctx* c, int source, int dist_type, int64_t n)
{
    for (auto& b : c->nj) {
        if (source == DPR_SRC_MSA) {
            if (int rc = msa_dist_rows(c->msa, b, dist_type, c->stream)) return rc;
        } else if (source == DPR_SRC_MASH) {
            if (b.world > 1) {
                if (int rc = mash_dist_matrix_sharded(c->mash, b.rank, b.world, b.rows_local, b.D, b.ld, c->stream)) return rc;
            } else {
                for (int64_t r0 = 0; r0 < b.rows_local; r0 += 32768) {
                    const int64_t nr = b.rows_local - r0 < 32768 ? b.rows_local - r0 : 32768;
                    if (int rc = mash_dist_rows(c->mash, r0, nr, b.rank, b.world, true, n, b.D + r0 * b.ld, b.ld, c->stream)) return rc;
                }
            }
        } else {
            if (int rc = nj_expand_lower(b, c->packed_lower, c->stream)) return rc;
        }
        if (c->plan.kind == DPR_NJ_PLAN_BIONJ)
            if (int rc = nj_bionj_init(b, c->stream)) return rc;
    }
    return DPR_OK;
}
// row sums of the own rows: into U (whole matrix here), the slice of the legacy exchange, or the window's slice (windows set up:
// every rank then reads the other ranks' sums straight from their windows, behind one barrier); then Ur and the keys
static int dist_row_sums(dpr_ctx* c)
{
    const bool dealt = c->plan.rows_dealt(), windows = dealt && c->plan.exchange != kNjsLegacy;
    for (auto& b : c->nj)
        if (int rc = nj_init_sums(b, c->stream, !dealt ? nullptr : windows ? reinterpret_cast<double*>(b.peer.win + b.peer.lay.off_slice) : b.slice)) return rc;
    if (dealt)
        if (int rc = windows ? njs_barrier(c) : exchange(c, EX_U)) return rc;
    for (auto& b : c->nj) {
        if (dealt)
            if (int rc = windows ? njs_launch_unpack_u(b, c->stream) : nj_launch_unpack_u(b, c->stream)) return rc;
        if (int rc = nj_prepare(b, c->stream)) return rc;
    }
    return DPR_OK;
}
// rows-pruned plan: the epoch state of njr.hip on every rank held here
static int dist_build_njr(dpr_ctx* c)
{
    // exchange plan of the loop: -1 / 0 = default (collective -- all-gathers -- with RCCL and between virtual ranks; mailbox for
    // ranks joined without RCCL), 1 = collective, 2 = mailbox
    int rplan = c->nj_exchange == 2 ? kNjrMailbox : c->nj_exchange == 1 ? kNjrCollective : (c->local_comm ? kNjrMailbox : kNjrCollective);
    if (c->nj_exchange < 0 && !c->local_comm)
        if (const char* e = std::getenv("DPR_NJ_EXCHANGE")) rplan = std::strcmp(e, "mailbox") == 0 ? kNjrMailbox : kNjrCollective;
    if (rplan == kNjrCollective && c->vworld == 0 && !comm_real(c)) { set_error("dpr_dist_matrix: the collective plan of the row-sharded pruned NJ needs a transport between the ranks (RCCL, or dpr_comm_init_shared)"); return DPR_ERR_STATE; }
    for (auto& b : c->nj) {
        b.rs.world = c->world; b.rs.rank = b.rank; b.rs.plan = rplan;
        b.rs.win_off = b.peer.lay.off_njr;
        b.rs.gather = njr_gather_cb; b.rs.cb_ctx = c;
        // (ranks on the shared region's windows: with the mailbox plan the barrier runs through the njr windows, no callback;
        //  with the collective plan through the region)
        b.rs.barrier = (c->vworld == 0 && (c->comm || (c->shm && rplan == kNjrCollective))) ? njr_barrier_cb : nullptr;
        b.rs.launches = 0; b.rs.collectives = 0;
    }
    std::vector<NjBuffers*> ranks = njr_ranks(c);
    if (int rc = njr_build(ranks, c->stream)) return rc;
    c->nj_exchange_note = std::string("row-sharded pruned NJ (njr.hip), exchange plan ") + (rplan == kNjrMailbox ? "mailbox" : "collective");
    return DPR_OK;
}
// the pruned plans on a whole copy: who shares the unit tests and scans of an iteration -- the real ranks (unit-sharded), emulated
// ones (virtual shards), or nobody
static void njp_set_shards(dpr_ctx* c, int kind)
{
    NjPruned& q = c->nj[0].pr;
    if (kind == DPR_NJ_PLAN_UNIT_SHARDED) { q.sh_world = c->world; q.sh_rank = c->rank; q.sh_virtual = false; q.gather = njp_gather_cb; q.gather_ctx = c; }
    else if (ctx_vshards(c) > 1) { q.sh_world = ctx_vshards(c); q.sh_rank = 0; q.sh_virtual = true; }
}
static int dist_build_njp(dpr_ctx* c)
{
    NjPruned& q = c->nj[0].pr;
    njp_set_shards(c, c->plan.kind);
    if (c->nj_adaptive >= 0) q.adaptive = c->nj_adaptive;
    if (int rc = njp_build(c->nj[0], c->stream)) return rc;
    if (c->nj_adaptive >= 0) q.adaptive = c->nj_adaptive;      // (the explicit setting wins over the environment)
    return DPR_OK;
}
static bool plan_is_njp(int kind) { return kind == DPR_NJ_PLAN_SINGLE_PRUNED || kind == DPR_NJ_PLAN_REPLICAS || kind == DPR_NJ_PLAN_UNIT_SHARDED; }

}  // namespace dpr

using namespace dpr;

__global__ void dpr_warm_kernel(int x);

extern "C" {

// ---- distance matrix ----------------------------------------------------------------------------------
int dpr_dist_matrix(dpr_ctx* c, int source, int dist_type, int k)
{
    if (!c) { set_error("dpr_dist_matrix: null ctx"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    if (c->world > 1 && c->vworld == 0 && !c->comm && !c->local_comm && !c->shm) { set_error("dpr_dist_matrix: dpr_comm_init was not called"); return DPR_ERR_STATE; }
    int64_t n = 0;
    if (source == DPR_SRC_MSA) {
        if (!c->msa.planes) { set_error("dpr_dist_matrix: call dpr_set_msa first"); return DPR_ERR_STATE; }
        n = c->msa.n;
    } else if (source == DPR_SRC_MATRIX) {
        if (!c->packed_lower) { set_error("dpr_dist_matrix: call dpr_set_matrix_lower first"); return DPR_ERR_STATE; }
        n = c->n_input;
    } else if (source == DPR_SRC_MASH) {
        if (!c->mash.sketches) { set_error("dpr_dist_matrix: call dpr_set_reads and dpr_sketch first"); return DPR_ERR_STATE; }
        if (k != c->mash.k) { set_error("dpr_dist_matrix: k differs from the sketch k"); return DPR_ERR_ARG; }
        n = c->mash.n;
    } else {
        set_error("dpr_dist_matrix: source not available");
        return DPR_ERR_ARG;
    }
    const int kind = ctx_nj_plan(c, n, "dpr_dist_matrix");
    if (kind < 0) return kind;
    c->have_matrix = 0;
    c->plan = NjPlan{ kind, kNjsLegacy };
    c->nj_exchange_note.clear();
    if (int rc = dist_alloc(c, n)) return rc;
    DPR_HIP(hipEventRecord(c->ev[0], c->stream));
    if (int rc = dist_fill(c, source, dist_type, n)) return rc;
    if (int rc = dist_row_sums(c)) return rc;
    if (int rc = kind == DPR_NJ_PLAN_ROWS_PRUNED ? dist_build_njr(c) : plan_is_njp(kind) ? dist_build_njp(c) : DPR_OK) return rc;
    DPR_HIP(hipEventRecord(c->ev[1], c->stream));
    DPR_HIP(hipStreamSynchronize(c->stream));
    float ms = 0;
    DPR_HIP(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->dist_ms = ms;
    c->have_matrix = 1;   // (the packed triangle of a MATRIX source stays until dpr_set_matrix_lower / dpr_destroy)
    return DPR_OK;
}

// Allocate the N x N matrix buffers of a following dpr_dist_matrix(n tips) now (single-rank contexts; a no-op
// otherwise): dpr_dist_matrix finds them in place.  The CLI calls it from its device thread as soon as the number of
// input sequences is known, while the host threads are still packing them.
int dpr_reserve_nj(dpr_ctx* c, int64_t n)
{
    if (!c || n < 2 || n >= (1 << 24)) { set_error("dpr_reserve_nj: bad argument"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    const int kind = ctx_nj_plan(c, n, "dpr_reserve_nj");
    if (kind < 0) return kind;
    // (only the plans of one rank on its own copy: the others allocate together, in dpr_dist_matrix)
    if (kind != DPR_NJ_PLAN_SINGLE_STREAM && kind != DPR_NJ_PLAN_SINGLE_PRUNED && kind != DPR_NJ_PLAN_BIONJ) return DPR_OK;
    c->have_matrix = 0;
    if (int rc = nj_alloc(c->nj[0], n, 0, 1, c->stream, 0, kind == DPR_NJ_PLAN_BIONJ)) return rc;
    if (kind == DPR_NJ_PLAN_SINGLE_PRUNED) {
        njp_set_shards(c, kind);
        if (int rc = njp_arena(c->nj[0].pr, n, c->stream)) return rc;
    }
    DPR_HIP(hipStreamSynchronize(c->stream));
    return DPR_OK;
}

// The first hipGraph of a process costs 10-30 ms to instantiate (the next ones 0.2 ms); the pruned NJ replays graphs, so that
// cost would sit in front of its first 32 iterations with the GPU idle.  The CLI calls this from its device thread, after the
// allocations and the upload that were waiting for the context.  It runs on the context's own stream and, like every other
// entry point, must be the only call on its context: a private stream (which let it run beside other calls) is a second
// hardware queue, 9-16 ms to create, and what ran beside it queued behind the runtime's locks anyway.
// Safe to call any number of times.
int dpr_warm_graphs(dpr_ctx* c)
{
    if (!c) { set_error("dpr_warm_graphs: null ctx"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    const bool tlog = log_level("cli") > 0;
    const auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (tlog) std::fprintf(stderr, "  dpr_warm_graphs: %s at %.1f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    };
    hipStream_t st = c->stream;
    if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
        hipLaunchKernelGGL(dpr_warm_kernel, dim3(1), dim3(64), 0, st, 0);
        ScopedGraph g;
        ScopedGraphExec ge;
        if (hipStreamEndCapture(st, g.put()) == hipSuccess && g) {
            if (hipGraphInstantiate(ge.put(), g, nullptr, nullptr, 0) == hipSuccess && ge) {
                lap("first hipGraphInstantiate");
                (void)hipGraphLaunch(ge, st);
                (void)hipStreamSynchronize(st);
                lap("graph replayed");
            }
        }
    }
    // ... and of its staged copies: the first device-to-host copy of more than a few KB into pageable memory costs 7.7 ms
    // (staging buffers); without this it is the first epoch rebuild of the NJ run that pays (240 KB of row sums)
    {
        DevBuf<char> d;
        constexpr size_t kWarmBytes = 512 << 10;
        if (d.alloc(kWarmBytes) == hipSuccess) {
            std::vector<char> h(kWarmBytes);
            (void)hipMemsetAsync(d, 0, kWarmBytes, st);
            (void)hipStreamSynchronize(st);
            // (asynchronous copies on the context's stream: a synchronous hipMemcpy runs on the NULL stream, which serialises
            //  with every blocking stream of the device; pageable staging is exercised all the same)
            (void)hipMemcpyAsync(h.data(), d, kWarmBytes, hipMemcpyDeviceToHost, st);
            (void)hipStreamSynchronize(st);
            (void)hipMemcpyAsync(d, h.data(), kWarmBytes, hipMemcpyHostToDevice, st);
            (void)hipStreamSynchronize(st);
        }
    }
    lap("staged copies both ways");
    (void)hipGetLastError();
    return DPR_OK;
}

// ---- NJ -------------------------------------------------------------------------------------------------
} // extern "C" (helper)
namespace dpr {
int fetch_state(dpr_ctx* c, NjState* st)
{
    DPR_HIP(hipMemcpyAsync(st, c->nj[0].st, sizeof(NjState), hipMemcpyDeviceToHost, c->stream));
    DPR_HIP(hipStreamSynchronize(c->stream));
    return DPR_OK;
}
}  // namespace dpr
extern "C" {

int64_t dpr_nj_run(dpr_ctx* c, int64_t max_iters, int32_t* merge_x, int32_t* merge_y, double* bl_x,
                   double* bl_y, double* last_d)
{
    if (!c || !c->have_matrix) { set_error("dpr_nj_run: call dpr_dist_matrix first"); return DPR_ERR_STATE; }
    DPR_HIP(hipSetDevice(c->device));
    NjState st;
    if (int rc = fetch_state(c, &st)) return rc;
    int64_t todo = st.n - 2;
    if (todo < 0) todo = 0;
    if (max_iters >= 0 && max_iters < todo) todo = max_iters;
    const int64_t it0 = st.it;
    c->nj[0].kt = &c->nj_kt;
    if (c->nj_kt.stride > 0 && it0 == 0) { c->nj_kt.samples = 0; for (double& v : c->nj_kt.us_sum) v = 0; }
    c->nj_launches = 0; c->nj_collectives = 0;
    DPR_HIP(hipEventRecord(c->ev[2], c->stream));
    if (c->plan.kind == DPR_NJ_PLAN_ROWS_PRUNED) {
        std::vector<NjBuffers*> ranks = njr_ranks(c);
        c->nj[0].rs.launches = 0; c->nj[0].rs.collectives = 0;
        if (int rc = njr_run(ranks, it0, todo, c->stream)) return rc;
        c->nj_launches = c->nj[0].rs.launches; c->nj_collectives = c->nj[0].rs.collectives;
    } else if (plan_is_njp(c->plan.kind)) {
        if (int rc = njp_run(c->nj[0], it0, todo, c->stream)) return rc;
    } else {
        for (int64_t k = 0; k < todo; ++k)
            if (int rc = nj_iteration(c, st.n - k, it0 + k)) return rc;
    }
    DPR_HIP(hipEventRecord(c->ev[3], c->stream));       // (the loop itself: the barrier + flush below are once per run)
    if (c->plan.one_exchange_loop()) {
        // every rank must be through its pulls of the last iteration before an owner flushes the last row buffers
        if (int rc = njs_barrier(c)) return rc;
        for (auto& b : c->nj)
            if (int rc = njs_launch_finish(b, st.n - todo, it0 + todo, c->njs_pending, c->stream)) return rc;
        c->njs_pending = false;
        if (int rc = njs_barrier(c)) return rc;      // the flushed rows may be read by other ranks (final distance, hooks)
    } else {
        for (auto& b : c->nj)
            if (!b.pr.active)
                if (int rc = nj_launch_finish(b, st.n - todo, it0 + todo, c->stream)) return rc;
    }
    if (int rc = fetch_state(c, &st)) return rc;
    float ms = 0;
    DPR_HIP(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    c->nj_ms = ms;
    if (!c->nj_kt.ev.empty()) {       // per-kernel timing samples of this run (stream idle)
        NjKernelTiming& kt = c->nj_kt;
        const size_t grp = (size_t)kt.nk + 1;
        for (size_t g0 = 0; kt.nk > 0 && g0 + grp <= kt.ev.size(); g0 += grp) {
            for (int k = 0; k < kt.nk; ++k) {
                float us = 0;
                if (hipEventElapsedTime(&us, kt.ev[g0 + (size_t)k], kt.ev[g0 + (size_t)k + 1]) == hipSuccess) kt.us_sum[k] += (double)us * 1e3;
            }
            ++kt.samples;
        }
        for (hipEvent_t e : kt.ev) (void)hipEventDestroy(e);
        kt.ev.clear();
    }
    const int64_t done = st.it - it0;
    if (done > 0) {
        if (merge_x) DPR_HIP(hipMemcpy(merge_x, c->nj[0].log_x + it0, sizeof(int32_t) * (size_t)done, hipMemcpyDeviceToHost));
        if (merge_y) DPR_HIP(hipMemcpy(merge_y, c->nj[0].log_y + it0, sizeof(int32_t) * (size_t)done, hipMemcpyDeviceToHost));
        if (bl_x) DPR_HIP(hipMemcpy(bl_x, c->nj[0].log_bx + it0, sizeof(double) * (size_t)done, hipMemcpyDeviceToHost));
        if (bl_y) DPR_HIP(hipMemcpy(bl_y, c->nj[0].log_by + it0, sizeof(double) * (size_t)done, hipMemcpyDeviceToHost));
    }
    if (st.status == 3) {
        set_error("dpr_nj_run: the exchange between the ranks failed (a rank's record did not arrive within the poll limit, or the all-gather delivered a stale one)");
        return DPR_ERR_COMM;
    }
    if (st.status == 4) {
        // (njs_post_kernel left the two differing words in st.q / st.d and the ranks in st.x / st.y)
        char msg[320];
        std::snprintf(msg, sizeof msg, "dpr_nj_run: the ranks' replicated row sums differ after %lld iterations (rank %d: %a, rank %d: %a): a row pulled from its owner "
                      "was stale or torn -- the merge log up to here is not trustworthy; use the legacy exchange (dpr_ctx_set_nj_exchange(ctx, 0))",
                      (long long)st.it, (int)st.x, st.q, (int)st.y, st.d);
        set_error(msg);
        return DPR_ERR_COMM;
    }
    if (st.status == 5) {
        set_error("dpr_nj_run: internal: the test blocks of the post kernel did not see the producer blocks' tag within 2 ms (njp_post2_kernel; DPR_NJP_POST2=0 selects the fused kernel)");
        return DPR_ERR_HIP;
    }
    if (st.status != 0) {
        set_error("dpr_nj_run: no Q candidate below the reference's init value 10000 (undefined in the reference)");
        return DPR_ERR_NOCAND;
    }
    if (last_d && st.n == 2) {
        // D[0][1] of the final pair (src/neighborJoining.cu:245-249): the row of slot 1, at the column of slot 0.  (Rows-pruned plan:
        // every rank's finish kernel has run -- njr_run ends with a barrier over the ranks behind the finish launches; one-exchange
        // loop: the owner's flush is behind the barrier above)
        NjBuffers& b0 = c->nj[0];
        int32_t pos01[2] = { 0, 1 };
        if (b0.pr.in_positions()) DPR_HIP(hipMemcpy(pos01, b0.pr.pos_of_slot, sizeof(pos01), hipMemcpyDeviceToHost));
        const double* row1 = slot_row(c, 1, pos01[1], true);
        // real ranks on the legacy exchange hold no mapping of each other's rows: the owner sends the value in a record, and every
        // rank, the owner included, takes part in that all-gather
        const bool by_record = c->plan.rows_dealt() && c->vworld == 0 && c->plan.exchange == kNjsLegacy;
        if (row1 && !by_record) {
            DPR_HIP(hipMemcpy(last_d, row1 + pos01[0], sizeof(double), hipMemcpyDeviceToHost));
        } else {
            NjRecord rec{ 0.0, 0ull, 0.0, 0ull };
            if (row1) DPR_HIP(hipMemcpy(&rec.d, row1 + pos01[0], sizeof(double), hipMemcpyDeviceToHost));
            DPR_HIP(hipMemcpy(b0.recs + c->rank, &rec, sizeof(NjRecord), hipMemcpyHostToDevice));
            if (int rc = exchange(c, EX_RECS)) return rc;
            DPR_HIP(hipStreamSynchronize(c->stream));
            DPR_HIP(hipMemcpy(&rec, b0.recs + 0, sizeof(NjRecord), hipMemcpyDeviceToHost));
            *last_d = rec.d;
        }
    }
    return done;
}

int dpr_argmin_once(dpr_ctx* c, int reps, int32_t* out_i, int32_t* out_j, double* out_q, float* out_ms)
{
    if (!c || !c->have_matrix) { set_error("dpr_argmin_once: call dpr_dist_matrix first"); return DPR_ERR_STATE; }
    DPR_HIP(hipSetDevice(c->device));
    if (reps < 1) reps = 1;
    NjState st0;
    if (int rc = fetch_state(c, &st0)) return rc;
    // pruned mode: the streaming kernel runs over the position-space matrix (all P positions, dead
    // ones carry NaN row sums); it = 0 because the bounds kernel already finished U[x]
    auto probe = [&](NjBuffers& b) -> int {
        return b.pr.in_positions() ? nj_launch_scan(b, true, b.pr.P, 0, c->stream) : nj_launch_scan(b, true, st0.n, st0.it, c->stream);
    };
    for (auto& b : c->nj)
        if (int rc = probe(b)) return rc;  // warm
    DPR_HIP(hipEventRecord(c->ev[2], c->stream));
    for (int r = 0; r < reps; ++r)
        for (auto& b : c->nj)
            if (int rc = probe(b)) return rc;
    DPR_HIP(hipEventRecord(c->ev[3], c->stream));
    for (auto& b : c->nj)
        if (int rc = nj_launch_select_local(b, nj_scan_grid(), c->stream)) return rc;
    if (int rc = exchange(c, EX_RECS)) return rc;
    const int ew = c->plan.whole_matrix() ? 1 : c->world;      // ranks whose records differ
    std::vector<NjRecord> recs((size_t)ew);
    DPR_HIP(hipMemcpyAsync(recs.data(), c->nj[0].recs, sizeof(NjRecord) * (size_t)ew, hipMemcpyDeviceToHost, c->stream));
    DPR_HIP(hipStreamSynchronize(c->stream));
    float ms = 0;
    DPR_HIP(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    if (out_ms) *out_ms = ms / (float)reps;
    const int w = dpr_record_reduce(recs.data(), ew);
    if (w < 0 || !(recs[(size_t)w].q < 10000.0)) { set_error("dpr_argmin_once: no Q candidate below 10000"); return DPR_ERR_NOCAND; }
    const NjRecord& rec = recs[(size_t)w];
    if (out_i) *out_i = (int32_t)(rec.key & 0xFFFFFFull);
    if (out_j) *out_j = (int32_t)((rec.key >> 24) & 0xFFFFFFull);
    if (out_q) *out_q = rec.q;
    return DPR_OK;
}

// the one place that chooses a plan; the table is in include/dipper_hip.h
int dpr_nj_plan_resolve(int world, int virtual_ranks, int variant, int pruned, int multi_plan, int virtual_shards, int64_t n, uint64_t total_bytes)
{
    if (world < 1 || variant < 0 || variant > 1 || multi_plan < 0 || multi_plan > 3 || virtual_shards < 1 || n < 2) { set_error("dpr_nj_plan_resolve: bad argument"); return DPR_ERR_ARG; }
    if (variant == 1) {
        if (!virtual_ranks && virtual_shards == 1) return DPR_NJ_PLAN_BIONJ;
        set_error("BIONJ runs the single-rank streaming plan: not on a context of virtual ranks or with virtual shards (dpr_set_nj_virtual_shards > 1)");
        return DPR_ERR_ARG;
    }
    if (!pruned || n < 3) return world > 1 ? DPR_NJ_PLAN_ROWS_STREAM : DPR_NJ_PLAN_SINGLE_STREAM;
    if (world == 1) return DPR_NJ_PLAN_SINGLE_PRUNED;
    if (multi_plan == 3) return DPR_NJ_PLAN_ROWS_PRUNED;
    if (virtual_ranks) return DPR_NJ_PLAN_ROWS_STREAM;       // (a context of virtual ranks keeps no whole copy per rank)
    // auto: the two epoch buffers of a whole copy (2 x 8 n^2 bytes) no longer fit this device: deal the rows
    if (multi_plan == 0 && 2.0 * 8.0 * (double)n * (double)n > 0.85 * (double)total_bytes) return DPR_NJ_PLAN_ROWS_PRUNED;
    return multi_plan == 1 || (multi_plan == 0 && n >= kNjShardTips) ? DPR_NJ_PLAN_UNIT_SHARDED : DPR_NJ_PLAN_REPLICAS;
}

int dpr_njp_unit_owner(int64_t strip, int64_t group, int64_t P, int world) { return njp_unit_owner(strip, group, P, world); }

// validation knob: the next dpr_dist_matrix on a single-rank context sets up `w` emulated unit-sharded ranks
int dpr_set_nj_virtual_shards(int w)
{
    if (w < 1 || w > 64) { set_error("dpr_set_nj_virtual_shards: 1 <= w <= 64"); return DPR_ERR_ARG; }
    g_nj_vshards = w;
    return DPR_OK;
}

int dpr_set_nj_multi_plan(int plan)
{
    if (plan < 0 || plan > 3) { set_error("dpr_set_nj_multi_plan: 0 auto, 1 unit-sharded, 2 single-GPU plan on every rank, 3 row-sharded pruned"); return DPR_ERR_ARG; }
    g_nj_multi_plan = plan;
    return DPR_OK;
}
int dpr_nj_is_unit_sharded(dpr_ctx* c) { return c && c->plan.kind == DPR_NJ_PLAN_UNIT_SHARDED ? 1 : 0; }
// the multi-rank NJ plan the last dpr_dist_matrix set up, in words (the CLI prints it; tests assert on it)
int dpr_get_nj_multi_info(dpr_ctx* c, char* buf, int cap)
{
    if (!c || !buf || cap <= 0) { set_error("dpr_get_nj_multi_info: bad argument"); return DPR_ERR_ARG; }
    static const char* const ex[] = { "legacy (two all-gathers per iteration)", "peer (one all-gather, rows pulled)", "mailbox (no collective)" };
    std::string s = "single rank";
    switch (c->plan.kind) {
    case DPR_NJ_PLAN_BIONJ: if (c->world > 1) s = "BIONJ, streaming, every rank its own copy"; break;
    case DPR_NJ_PLAN_ROWS_PRUNED: s = c->nj_exchange_note; break;
    case DPR_NJ_PLAN_UNIT_SHARDED: s = "pruned, matrix replicated, unit tests and scans sharded (one all-gather of block records per iteration)"; break;
    case DPR_NJ_PLAN_REPLICAS: s = "pruned, every rank runs the single-GPU plan on its own copy of the matrix (replicas)"; break;
    case DPR_NJ_PLAN_ROWS_STREAM: s = std::string("streaming, rows sharded block-cyclically, exchange ") + ex[c->plan.exchange >= 0 && c->plan.exchange <= 2 ? c->plan.exchange : 0]; break;
    }
    std::snprintf(buf, (size_t)cap, "%s", s.c_str());
    return DPR_OK;
}

// the same three knobs for ONE context (two contexts in one process may run different plans); value -1 = follow
// the process-wide default again.  Take effect at the context's next dpr_dist_matrix.
int dpr_ctx_set_nj_mode(dpr_ctx* c, int mode)
{
    if (!c || mode < -1 || mode > 1) { set_error("dpr_ctx_set_nj_mode: mode must be -1, 0 or 1"); return DPR_ERR_ARG; }
    c->nj_mode = mode;
    return DPR_OK;
}
int dpr_ctx_set_nj_multi_plan(dpr_ctx* c, int plan)
{
    if (!c || plan < -1 || plan > 3) { set_error("dpr_ctx_set_nj_multi_plan: -1 default, 0 auto, 1 unit-sharded, 2 single-GPU plan on every rank, 3 row-sharded pruned"); return DPR_ERR_ARG; }
    c->nj_multi_plan = plan;
    return DPR_OK;
}
// 0 = NJ, 1 = BIONJ (include/dipper_hip.h); read by the context's next dpr_dist_matrix / dpr_reserve_nj
int dpr_ctx_set_nj_variant(dpr_ctx* c, int variant)
{
    if (!c || variant < 0 || variant > 1) { set_error("dpr_ctx_set_nj_variant: variant must be 0 (NJ) or 1 (BIONJ)"); return DPR_ERR_ARG; }
    c->nj_variant = variant;
    return DPR_OK;
}
int dpr_get_nj_lambda(dpr_ctx* c, double* out, int64_t* count)
{
    if (!c || !count) { set_error("dpr_get_nj_lambda: null argument"); return DPR_ERR_ARG; }
    if (!c->have_matrix || c->plan.kind != DPR_NJ_PLAN_BIONJ || !c->nj[0].log_lam) { set_error("dpr_get_nj_lambda: no BIONJ matrix (dpr_ctx_set_nj_variant(ctx, 1), then dpr_dist_matrix)"); return DPR_ERR_STATE; }
    DPR_HIP(hipSetDevice(c->device));
    NjState st;
    if (int rc = fetch_state(c, &st)) return rc;
    *count = st.it;
    if (out && st.it > 0) DPR_HIP(hipMemcpy(out, c->nj[0].log_lam, sizeof(double) * (size_t)st.it, hipMemcpyDeviceToHost));
    return DPR_OK;
}
// Per-kernel timing of the pruned NJ loop: stride > 0 makes the following dpr_nj_run calls enqueue their iterations
// eagerly (no hipGraph replay) with HIP events on the library's stream around the launches of every stride-th iteration.
int dpr_ctx_set_nj_kernel_timing(dpr_ctx* c, int stride)
{
    if (!c || stride < 0) { set_error("dpr_ctx_set_nj_kernel_timing: stride >= 0"); return DPR_ERR_ARG; }
    c->nj_kt.stride = stride;
    return DPR_OK;
}
int dpr_get_nj_kernel_timing(dpr_ctx* c, int* kernels, double* us_avg, int64_t* samples)
{
    if (!c) { set_error("dpr_get_nj_kernel_timing: null ctx"); return DPR_ERR_ARG; }
    if (kernels) *kernels = c->nj_kt.nk;
    if (samples) *samples = c->nj_kt.samples;
    if (us_avg) for (int k = 0; k < kNjKernelsMax; ++k) us_avg[k] = c->nj_kt.samples > 0 ? c->nj_kt.us_sum[k] / (double)c->nj_kt.samples : 0.0;
    return DPR_OK;
}
const char* dpr_nj_kernel_name(int idx) { return njp_kernel_name(idx); }
int dpr_get_nj_phase_stamps(uint64_t* out) { return njp_phase_stamps((unsigned long long*)out); }
int dpr_get_njp_list(dpr_ctx* c, int32_t* out, int64_t cap, int64_t* count, int64_t* positions, double* ur, int64_t ur_cap)
{
    if (!c || !out || !count || !positions) { set_error("dpr_get_njp_list: null argument"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    return njp_debug_list(c->nj[0], out, cap, count, positions, ur, ur_cap);
}

int dpr_ctx_set_nj_virtual_shards(dpr_ctx* c, int w)
{
    if (!c || w < -1 || w == 0 || w > 64) { set_error("dpr_ctx_set_nj_virtual_shards: -1 or 1 <= w <= 64"); return DPR_ERR_ARG; }
    c->nj_vshards = w;
    return DPR_OK;
}

// 0 = full streaming scan every iteration, 1 = exact pruned scan (default)
int dpr_set_nj_mode(int mode)
{
    if (mode != 0 && mode != 1) { set_error("dpr_set_nj_mode: mode must be 0 or 1"); return DPR_ERR_ARG; }
    g_nj_mode = mode;
    return DPR_OK;
}

// Adaptive plan of the single-rank NJ (default on): the exact pruned scan while its bounds prune; hand-over to the streaming
// loop once more than 70 % of an epoch's units are listed per iteration, pruned probes with back-off (see dpr_internal.hpp).  The
// merge log does not depend on it.  on = 0: pruned scans only; -1: DPR_NJ_ADAPTIVE / default.  Takes effect at the next
// dpr_dist_matrix.
int dpr_ctx_set_nj_adaptive(dpr_ctx* c, int on)
{
    if (!c || on < -1 || on > 1) { set_error("dpr_ctx_set_nj_adaptive: -1, 0 or 1"); return DPR_ERR_ARG; }
    c->nj_adaptive = on;
    return DPR_OK;
}
// iterations that ran as streaming scans and epochs that switched, since the matrix was built
int dpr_get_nj_adaptive_stats(dpr_ctx* c, int64_t* stream_iterations, int64_t* stream_epochs)
{
    if (!c || !c->have_matrix || !c->nj[0].pr.active) { set_error("dpr_get_nj_adaptive_stats: pruned path not active"); return DPR_ERR_STATE; }
    if (stream_iterations) *stream_iterations = c->nj[0].pr.stream_iterations;
    if (stream_epochs) *stream_epochs = c->nj[0].pr.stream_epochs;
    return DPR_OK;
}

// units scanned by the pruned path since the matrix was built, and units per full scan
int dpr_get_prune_stats(dpr_ctx* c, uint64_t* units_scanned, uint64_t* units_per_full_scan)
{
    if (!c || !c->have_matrix || !c->nj[0].pr.active) { set_error("dpr_get_prune_stats: pruned path not active"); return DPR_ERR_STATE; }
    NjState st;
    if (int rc = fetch_state(c, &st)) return rc;
    if (units_scanned) *units_scanned = st.units_scanned;
    if (units_per_full_scan) *units_per_full_scan = (uint64_t)c->nj[0].pr.utot0;
    return DPR_OK;
}


int dpr_get_nj_progress(dpr_ctx* c, int64_t* iterations_done, int64_t* active)
{
    if (!c || !c->have_matrix) { set_error("dpr_get_nj_progress: call dpr_dist_matrix first"); return DPR_ERR_STATE; }
    DPR_HIP(hipSetDevice(c->device));
    NjState st;
    if (int rc = fetch_state(c, &st)) return rc;
    if (iterations_done) *iterations_done = st.it;
    if (active) *active = st.n;
    return DPR_OK;
}

// ---- host-only restatement of the streaming loop, NJ and BIONJ (the contract is in include/dipper_hip.h) --------------------
}  // extern "C" (helpers)
namespace {
// pairwise tree over 256 values, c[t] += c[t + s] for s = 128 .. 1 (block_tree256 of the kernels)
double host_tree256(double* c)
{
    for (int s = 128; s > 0; s >>= 1)
        for (int t = 0; t < s; ++t) c[t] = c[t] + c[t + s];
    return c[0];
}
// chunk partials folded by 256 classes (ascending), then the tree (finish_ux of the kernels)
double host_fold(const double* part, int64_t nchunk)
{
    double p[256];
    for (int t = 0; t < 256; ++t) {
        double acc = 0.0;
        for (int64_t c = t; c < nchunk; c += 256) acc += part[c];
        p[t] = acc;
    }
    return host_tree256(p);
}
}  // namespace
extern "C" {

int64_t dpr_nj_variant_host(int variant, const double* lower_rows, int64_t N, int64_t max_iters, int32_t* merge_x, int32_t* merge_y,
                            double* bl_x, double* bl_y, double* last_d, double* lambda)
{
    if ((variant != 0 && variant != 1) || N < 2 || N >= (1 << 24) || (N > 2 && (!lower_rows || !merge_x || !merge_y || !bl_x || !bl_y))) {
        set_error("dpr_nj_variant_host: bad argument");
        return DPR_ERR_ARG;
    }
    const bool bionj = variant == 1;
    const int64_t ld = N;
    std::vector<double> D((size_t)(N * ld), 0.0), V, U((size_t)N), Ur((size_t)N), part((size_t)((N + 255) / 256 + 1));
    for (int64_t i = 0; i < N; ++i)
        for (int64_t j = 0; j < i; ++j) D[(size_t)(i * ld + j)] = D[(size_t)(j * ld + i)] = lower_rows[i * (i - 1) / 2 + j];
    if (bionj) V = D;
    // initial row sums: 256 class partials (j == t mod 256, ascending, j != i), the tree
    for (int64_t i = 0; i < N; ++i) {
        double c[256];
        for (int t = 0; t < 256; ++t) {
            double acc = 0.0;
            for (int64_t j = t; j < N; j += 256)
                if (j != i) acc += D[(size_t)(i * ld + j)];
            c[t] = acc;
        }
        U[(size_t)i] = host_tree256(c);
    }
    int64_t it = 0;
    for (; it < N - 2; ++it) {
        if (max_iters >= 0 && it >= max_iters) break;
        const int64_t n = N - it, last = n - 1, nchunk = (n + 255) / 256;
        const double r = (double)(n - 2);
        for (int64_t i = 0; i < n; ++i) Ur[(size_t)i] = U[(size_t)i] / r;
        // selection: both orientations of every element of the strict lower triangle, strict '<' on q, ties by key
        double bq = 10000.0;
        uint64_t bk = ~0ull;
        for (int64_t a = 1; a < n; ++a) {
            const double* row = D.data() + a * ld;
            const double ua = Ur[(size_t)a];
            for (int64_t c = 0; c < a; ++c) {
                const double dv = row[c], uc = Ur[(size_t)c];
                const double q1 = (dv - ua) - uc, q2 = (dv - uc) - ua;
                if (q1 <= bq) { const uint64_t k = dpr_nj_key(a, c, n); if (q1 < bq || k < bk) { bq = q1; bk = k; } }
                if (q2 <= bq) { const uint64_t k = dpr_nj_key(c, a, n); if (q2 < bq || k < bk) { bq = q2; bk = k; } }
            }
        }
        if (bk == ~0ull || !(bq < 10000.0)) break;     // no candidate
        const int64_t ki = (int64_t)(bk & 0xFFFFFFull), kj = (int64_t)((bk >> 24) & 0xFFFFFFull);
        const int64_t x = ki < kj ? ki : kj, y = ki < kj ? kj : ki;
        const double d = D[(size_t)(y * ld + x)];
        const double bx0 = (d + U[(size_t)x] / r - U[(size_t)y] / r) * 0.5, by0 = d - bx0;
        double blX = bx0, blY = by0;
        if (blX < 0) { blY += blX; blX = 0; }
        if (blY < 0) { blX += blY; blY = 0; }
        merge_x[it] = (int32_t)x; merge_y[it] = (int32_t)y; bl_x[it] = blX; bl_y[it] = blY;
        double lam = 0.5, vxy = 0.0;
        if (bionj) {
            vxy = V[(size_t)(y * ld + x)];
            for (int64_t c = 0; c < nchunk; ++c) {
                double v[256];
                for (int t = 0; t < 256; ++t) {
                    const int64_t k = c * 256 + t;
                    v[t] = (k < n && k != x && k != y) ? V[(size_t)(y * ld + k)] - V[(size_t)(x * ld + k)] : 0.0;
                }
                part[(size_t)c] = host_tree256(v);
            }
            const double ssum = host_fold(part.data(), nchunk);
            lam = 0.5 + ssum / (2.0 * r * vxy);
            if (vxy == 0.0 || lam != lam) lam = 0.5;
            else if (lam < 0.0) lam = 0.0;
            else if (lam > 1.0) lam = 1.0;
            if (lambda) lambda[it] = lam;
        }
        // update: slot i < n, i not x or y; the new node takes slot x, the last slot moves to y
        for (int64_t c = 0; c < nchunk; ++c) {
            double v[256];
            for (int t = 0; t < 256; ++t) {
                const int64_t i = c * 256 + t;
                double val = 0.0;
                if (i < n && i != x && i != y) {
                    const double dxi = D[(size_t)(x * ld + i)], dyi = D[(size_t)(y * ld + i)];
                    double vnew = 0.0;
                    if (bionj) {
                        const double vxi = V[(size_t)(x * ld + i)], vyi = V[(size_t)(y * ld + i)];
                        const double a = dxi - bx0, b = dyi - by0;
                        val = b + lam * (a - b);
                        vnew = vyi + lam * (vxi - vyi) - (lam * (1.0 - lam)) * vxy;
                    } else {
                        val = (dxi + dyi - d) * 0.5;
                    }
                    if (i != last) {
                        const double far = D[(size_t)(last * ld + i)];
                        U[(size_t)i] = U[(size_t)i] + (-dxi - dyi + val);
                        D[(size_t)(x * ld + i)] = val; D[(size_t)(i * ld + x)] = val;
                        D[(size_t)(y * ld + i)] = far; D[(size_t)(i * ld + y)] = far;
                        if (bionj) {
                            const double vfar = V[(size_t)(last * ld + i)];
                            V[(size_t)(x * ld + i)] = vnew; V[(size_t)(i * ld + x)] = vnew;
                            V[(size_t)(y * ld + i)] = vfar; V[(size_t)(i * ld + y)] = vfar;
                        }
                    } else {
                        U[(size_t)y] = U[(size_t)last] + (-dxi - dyi + val);
                        D[(size_t)(x * ld + y)] = val; D[(size_t)(y * ld + x)] = val;
                        if (bionj) { V[(size_t)(x * ld + y)] = vnew; V[(size_t)(y * ld + x)] = vnew; }
                    }
                }
                v[t] = val;
            }
            part[(size_t)c] = host_tree256(v);
        }
        U[(size_t)x] = host_fold(part.data(), nchunk);
    }
    if (it == N - 2 && last_d) *last_d = D[(size_t)(1 * ld + 0)];
    return it;
}

int dpr_get_njp_shape(dpr_ctx* c, int64_t* positions, int* row_groups, int* strips, int* post2, int* scan_grid)
{
    if (!c || !c->have_matrix || !c->nj[0].pr.active) { set_error("dpr_get_njp_shape: no pruned NJ state"); return DPR_ERR_STATE; }
    return njp_shape(c->nj[0].pr, positions, row_groups, strips, post2, scan_grid);
}

}  // extern "C"
