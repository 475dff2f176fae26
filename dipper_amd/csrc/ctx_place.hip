// C ABI, tree builders that place tips: k-closest placement (batches of distance rows: place_rows.hpp; which of them run beside the
// tree kernels: place_policy.hpp), exact placement mode, divide-and-conquer, fixed-backbone placement; dpr_place_run,
// dpr_place_policy_run, dpr_place_exact_run, dpr_dc_run, dpr_place_fixed_set / _run and their getters.
#include "place_policy.hpp"
#include "place_rows.hpp"

#include <array>

using namespace dpr;

// ---- said once for the three tree builders --------------------------------------------------------------
// is `source` set up for n tips?  `fn` is the entry point's name for the message (dpr_dc_run turns a matrix away before it asks)
static int check_source(dpr_ctx* c, const char* fn, int source, int k, int64_t n)
{
    const std::string f(fn);
    if (source == DPR_SRC_MSA) {
        if (!c->msa.planes || c->msa.n != n) { set_error(f + ": call dpr_set_msa with n sequences first"); return DPR_ERR_STATE; }
    } else if (source == DPR_SRC_MASH) {
        if (!c->mash.sketches || c->mash.n != n) { set_error(f + ": call dpr_set_reads and dpr_sketch first"); return DPR_ERR_STATE; }
        if (k != c->mash.k) { set_error(f + ": k differs from the sketch k"); return DPR_ERR_ARG; }
    } else if (source == DPR_SRC_MATRIX) {
        if (!c->packed_lower || c->n_input != n) { set_error(f + ": call dpr_set_matrix_lower first"); return DPR_ERR_STATE; }
    } else { set_error(f + ": unknown source"); return DPR_ERR_ARG; }
    return DPR_OK;
}

// queries per batch of a block of distances from nq queries to all m backbone tips: the block stays below 2 GiB, between 256 and
// 8192 queries, a multiple of 256, no more than the queries there are (dpr_dc_run's assignment, dpr_place_fixed_run)
static int64_t query_batch(int64_t m, int64_t nq)
{
    int64_t Q = ((int64_t)1 << 31) / (8 * m) / 256 * 256;
    if (Q < 256) Q = 256;
    if (Q > 8192) Q = 8192;
    if (Q > (nq + 255) / 256 * 256) Q = (nq + 255) / 256 * 256;
    return Q;
}

// c->place for n tips again; the fixed backbone of dpr_place_fixed_set lived in the old arrays
static int rebuild_place(dpr_ctx* c, int64_t n, int64_t M = 0)
{
    c->pfix.valid = false;
    return place_alloc(c->place, n, M);
}

// An imported backbone must be a rooted binary tree: `first` tips, first - 1 internal nodes, 2 first - 2 edges = the slots
// [0, 4 first - 4) all in use.  The reference's scan reads head[e[slot]] of every slot below 4 num - 4
// (src/placement_close_k.cu:325-338): an unused slot (e = belong = -1: a trifurcating root, a polytomy) is an
// out-of-bounds read there; here it is an error, since the edge records (one per undirected edge, dense: 2 num - 2 after
// num tips) have no place for a missing edge either (advisor, round 5).
static int check_backbone_slots(const char* fn, int64_t first, const int32_t* e, const int32_t* belong)
{
    for (int64_t s = 0; s < 4 * first - 4; ++s)
        if (e[s] < 0 || belong[s] < 0) {
            set_error(std::string(fn) + ": the backbone is not a rooted binary tree (directed edge slot " + std::to_string(s) + " of " +
                      std::to_string(4 * first - 4) + " is unused: a trifurcating root or a polytomy); resolve it first");
            return DPR_ERR_ARG;
        }
    return DPR_OK;
}

// c->place_trace: a fresh zeroed [3n] for this run
static int reset_place_trace(dpr_ctx* c, int64_t n)
{
    if (c->place_trace) { (void)hipFree(c->place_trace); c->place_trace = nullptr; }
    DPR_HIP(hipMalloc(&c->place_trace, sizeof(double) * (size_t)(3 * n)));
    DPR_HIP(hipMemsetAsync(c->place_trace, 0, sizeof(double) * (size_t)(3 * n), c->stream));
    return DPR_OK;
}

// the adjacency arrays head[2n] e[8n] nxt[8n] belong[8n] len[8n] between the caller and c->place, on c->stream
static int copy_adjacency(dpr_ctx* c, int64_t n, bool to_device, int32_t* head, int32_t* e, int32_t* nxt, int32_t* belong, double* len)
{
    const PlaceBuffers& p = c->place;
    struct Arr { void* host; void* dev; size_t bytes; };
    const Arr arrs[] = { { head, p.head, sizeof(int32_t) * (size_t)(2 * n) }, { e, p.e, sizeof(int32_t) * (size_t)(8 * n) },
                         { nxt, p.nxt, sizeof(int32_t) * (size_t)(8 * n) }, { belong, p.belong, sizeof(int32_t) * (size_t)(8 * n) },
                         { len, p.len, sizeof(double) * (size_t)(8 * n) } };
    for (const Arr& a : arrs) {
        if (to_device) DPR_HIP(hipMemcpyAsync(a.dev, a.host, a.bytes, hipMemcpyHostToDevice, c->stream));
        else DPR_HIP(hipMemcpyAsync(a.host, a.dev, a.bytes, hipMemcpyDeviceToHost, c->stream));
    }
    return DPR_OK;
}

extern "C" {

// what is fixed for a placement run's overlap policy; the environment is read here, once
static PlacePolicy::Fixed place_policy_fixed(const dpr_ctx* c, int source)
{
    const bool ranks = comm_real(c) && source != DPR_SRC_MATRIX;      // several real ranks share every batch
    const char* e = std::getenv("DPR_PLACE_BATCH");
    return PlacePolicy::fixed_for(source == DPR_SRC_MASH, ranks, !c->comm, std::getenv("DPR_PLACE_NO_OVERLAP") != nullptr, place_multi_min(), e ? std::atoll(e) : 0);
}

// k-closest placement of tips [first, last) into c->place (findPlacementTree / addQuery loop,
// src/placement_close_k.cu:756-851,888-987; findBackboneTreeDC, src/divide_and_conquer/
// placement_close_k.cu:832-925): distance rows in batches from the row pipeline, each batch produced on the main stream or beside
// the previous batch's tree kernels as the overlap policy says (place_policy.hpp).
// first == 2 starts from the two-tip tree, otherwise the imported backbone is already in the arrays.
static int place_range_batches(dpr_ctx* c, RowPipeline& pipe, PlacePolicy& pol, int64_t first, int64_t last)
{
    PlaceBuffers& p = c->place;
    const int64_t R = pol.fixed().R;
    if (first == 2) {
        if (int rc = place_init_fresh(p, c->stream)) return rc;
        if (int rc = pipe.src.fill(1, 1, pipe.rows(0), pipe.ldb, 2, c->stream)) return rc;
        if (int rc = place_initial_tree(p, pipe.src.row_ptr(1, 1, pipe.rows(0), pipe.ldb), c->stream)) return rc;
    } else {
        if (int rc = place_import_backbone(p, first, c->stream)) return rc;
    }
    size_t k = 0;
    for (int64_t i0 = first; i0 < last; i0 += R, ++k) {
        const int64_t nr = last - i0 < R ? last - i0 : R;
        if (int rc = pipe.make_available(k, i0, nr, pol.ahead())) return rc;
        ++c->place_batches;
        // the next batch beside this batch's tree kernels?  (the timed rule alone makes the host wait, for batch k - 1)
        if (pol.needs_timings(i0, nr))
            while (pol.observed() < k) {
                double tree_ms = 0, dist_ms = 0;
                if (int rc = pipe.t.wait_batch(pol.observed(), &tree_ms, &dist_ms)) return rc;
                pol.observe(tree_ms, dist_ms);
            }
        if (pol.decide(i0, nr)) {
            const int64_t j0 = i0 + R;
            if (int rc = pipe.produce_beside(k + 1, j0, last - j0 < R ? last - j0 : R)) return rc;
            c->place_overlapped = true;
            ++c->place_batches_overlapped;
        }
        const double* rows = pipe.rows(k);
        if (pipe.timed()) { if (int rc = pipe.t.tree.begin(c->stream)) return rc; }
        if (pipe.src.source == DPR_SRC_MATRIX) {      // packed triangle: rows are not evenly spaced
            for (int64_t i = i0; i < i0 + nr; ++i)
                if (int rc = place_tip(p, pipe.src.row_ptr(i, i0, rows, pipe.ldb), i, c->place_trace, c->stream)) return rc;
        } else {
            if (int rc = place_tips(p, rows, pipe.ldb, i0, nr, c->place_trace, c->stream)) return rc;
        }
        if (pipe.timed()) { if (int rc = pipe.t.tree.end(c->stream)) return rc; }
        if (int rc = pipe.mark_consumed(k)) return rc;
    }
    return DPR_OK;
}

// the scope of one run: policy and row pipeline (with the run's timers) live here; both streams are drained and the run's figures read on success
// and on failure, and every event of the run is released with the scope
static int place_range(dpr_ctx* c, int source, int dist_type, int64_t first, int64_t last)
{
    c->place_overlapped = false;
    c->place_batches = 0; c->place_batches_overlapped = 0;
    c->place_dist_ms = 0; c->place_dist_busy_ms = 0;
    PlacePolicy pol(place_policy_fixed(c, source), last);
    RowPipeline pipe(c, source, dist_type);
    if (int rc = pipe.init(pol.fixed().R, last, pol.fixed().allowed)) return rc;
    const int rc = place_range_batches(c, pipe, pol, first, last);
    pipe.drain();
    pipe.t.finish(c);
    return rc;
}

// dist_ms: the part of the run the tree kernels could not proceed for want of distance rows (without overlap: the
// distance batches themselves; with overlap: the tree stream's waits for them); tree_ms: the rest of the run.
int dpr_get_place_timing(dpr_ctx* c, double* dist_ms, double* tree_ms)
{
    if (!c) { set_error("dpr_get_place_timing: null ctx"); return DPR_ERR_ARG; }
    if (dist_ms) *dist_ms = c->place_dist_ms;
    if (tree_ms) *tree_ms = c->nj_ms > c->place_dist_ms ? c->nj_ms - c->place_dist_ms : 0.0;
    return DPR_OK;
}

// overlap mode of the last placement run: *overlapped = 1 and *dist_busy_ms = time the distance batches were in flight on
// the second stream (concurrent with the tree kernels, so NOT a summand of the run's wall time); else 0 / 0
int dpr_get_place_overlap(dpr_ctx* c, int* overlapped, double* dist_busy_ms)
{
    if (!c) { set_error("dpr_get_place_overlap: null ctx"); return DPR_ERR_ARG; }
    if (overlapped) *overlapped = c->place_overlapped ? 1 : 0;
    if (dist_busy_ms) *dist_busy_ms = c->place_overlapped ? c->place_dist_busy_ms : 0.0;
    return DPR_OK;
}

// batches of the last placement run and how many of them were produced beside the previous batch's tree kernels (the per-batch
// overlap policy of place_range)
int dpr_get_place_policy(dpr_ctx* c, int64_t* batches, int64_t* overlapped_batches)
{
    if (!c) { set_error("dpr_get_place_policy: null ctx"); return DPR_ERR_ARG; }
    if (batches) *batches = c->place_batches;
    if (overlapped_batches) *overlapped_batches = c->place_batches_overlapped;
    return DPR_OK;
}

// the policy over a described run: the loop of place_range_batches without the device
int dpr_place_policy_run(int source, int world, int window_transport, int no_overlap, int64_t multi_min, int64_t first, int64_t last,
                         int64_t batch_rows, const double* tree_ms, const double* dist_alone_ms, int64_t batches, int32_t* beside)
{
    if (source < DPR_SRC_MSA || source > DPR_SRC_MATRIX || world < 1 || first < 2 || last < first || batches < 0 || (batches > 0 && (!tree_ms || !dist_alone_ms || !beside))) {
        set_error("dpr_place_policy_run: bad argument");
        return DPR_ERR_ARG;
    }
    PlacePolicy pol(PlacePolicy::fixed_for(source == DPR_SRC_MASH, world > 1 && source != DPR_SRC_MATRIX, window_transport != 0, no_overlap != 0, multi_min, batch_rows), last);
    const int64_t R = pol.fixed().R;
    if (batches != (last - first + R - 1) / R) { set_error("dpr_place_policy_run: tips [first, last) in batches of " + std::to_string(R) + " rows are " + std::to_string((last - first + R - 1) / R) + " batches"); return DPR_ERR_ARG; }
    size_t k = 0;
    for (int64_t i0 = first; i0 < last; i0 += R, ++k) {
        const int64_t nr = last - i0 < R ? last - i0 : R;
        if (pol.needs_timings(i0, nr))
            for (size_t b = pol.observed(); b < k; ++b) pol.observe(tree_ms[b], dist_alone_ms[b]);
        beside[k] = pol.ahead() ? 1 : 0;
        pol.decide(i0, nr);
    }
    return DPR_OK;
}

int dpr_place_run(dpr_ctx* c, int source, int dist_type, int k, int64_t first, int64_t n, int32_t* head,
                  int32_t* e, int32_t* nxt, int32_t* belong, double* len)
{
    if (!c || !head || !e || !nxt || !belong || !len || n < 3 || first < 2 || first > n) { set_error("dpr_place_run: bad argument"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    if (int rc = check_source(c, "dpr_place_run", source, k, n)) return rc;
    if (first > 2) { if (int rc = check_backbone_slots("dpr_place_run", first, e, belong)) return rc; }
    if (int rc = rebuild_place(c, n)) return rc;
    PlaceBuffers& p = c->place;
    if (int rc = reset_place_trace(c, n)) return rc;
    DPR_HIP(hipMemsetAsync(p.misc + 2, 0, 2 * sizeof(int32_t), c->stream));      // fallback counters of the four-tip launches (dpr_get_place_walks)
    if (first > 2) { if (int rc = copy_adjacency(c, n, true, head, e, nxt, belong, len)) return rc; }
    DPR_HIP(hipEventRecord(c->ev[2], c->stream));
    if (int rc = place_range(c, source, dist_type, first, n)) return rc;
    DPR_HIP(hipEventRecord(c->ev[3], c->stream));
    if (int rc = copy_adjacency(c, n, false, head, e, nxt, belong, len)) return rc;
    DPR_HIP(hipStreamSynchronize(c->stream));
    float ms = 0;
    DPR_HIP(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    c->nj_ms = ms;
    if (log_level("place") > 0) {
        int64_t st[6] = { 0, 0, 0, 0, 0, 0 };
        if (dpr_get_place_walks(c, nullptr, st) == DPR_OK)
            std::fprintf(stderr, "[place] closest-list walks of %lld tips: %lld slots reached in all, largest walk %lld, %lld beyond the 2 048-entry LDS queue, %lld from a node of degree > 3; "
                         "four-tip launches: %lld tips fell back to evaluating every slot (dirty set full), %lld (too many blocks to re-scan)\n",
                         (long long)(n - first), (long long)st[2], (long long)st[1], (long long)st[0], (long long)st[3], (long long)st[4], (long long)st[5]);
    }
    return DPR_OK;
}

// ---- exact placement mode -----------------------------------------------------------------------------
static int place_exact_attempt(dpr_ctx* c, int source, int dist_type, int k, int64_t n, int32_t* head, int32_t* e,
                               int32_t* nxt, int32_t* belong, double* len)
{
    if (!c || !head || !e || !nxt || !belong || !len || n < 3) { set_error("dpr_place_exact_run: bad argument"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    if (int rc = check_source(c, "dpr_place_exact_run", source, k, n)) return rc;
    if (int rc = rebuild_place(c, n)) return rc;
    if (int rc = exact_alloc(c->exact, n)) return rc;
    PlaceBuffers& p = c->place;
    ExactBuffers& x = c->exact;
    if (int rc = reset_place_trace(c, n)) return rc;
    // distance rows in batches of R+1: the step of tip i also runs the passes of tip i+1, so a batch
    // shares its last row with the next one
    const int64_t R = 256;
    const int64_t ldb = (n + 15) / 16 * 16;
    DevBuf<double> rows;
    if (source != DPR_SRC_MATRIX) DPR_HIP(rows.alloc((size_t)((R + 1) * ldb)));
    int64_t r0 = 1;
    const RowSource src{ c, source, dist_type };
    auto row_ptr = [&](int64_t i) { return src.row_ptr(i, r0, rows, ldb); };
    DPR_HIP(hipEventRecord(c->ev[2], c->stream));
    int rc = DPR_OK;
    while (!rc) {
        const int64_t nr = n - r0 < R + 1 ? n - r0 : R + 1;
        if (r0 > 1) rc = exact_adapt(x, c->stream);
        if (!rc) rc = src.fill(r0, nr, rows, ldb, r0 + nr, c->stream);
        if (!rc && r0 == 1) rc = exact_init(p, x, row_ptr(1), nr > 1 ? row_ptr(2) : nullptr, nr > 1, c->stream);
        for (int64_t i = r0 < 2 ? 2 : r0; !rc && i < r0 + nr - 1; ++i) rc = exact_tip(p, x, i, row_ptr(i + 1), true, c->place_trace, c->stream);
        if (rc) break;
        if (r0 + nr == n) { rc = exact_tip(p, x, n - 1, nullptr, false, c->place_trace, c->stream); break; }
        r0 = r0 + nr - 1;
    }
    if (!rc) {
        DPR_HIP(hipEventRecord(c->ev[3], c->stream));
        rc = copy_adjacency(c, n, false, head, e, nxt, belong, len);
    }
    const hipError_t se = hipStreamSynchronize(c->stream);     // (the stream is idle before the scope releases the rows)
    if (rc) return rc;
    DPR_HIP(se);
    float ms = 0;
    DPR_HIP(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
    c->nj_ms = ms;
    return DPR_OK;
}

int dpr_place_exact_run(dpr_ctx* c, int source, int dist_type, int k, int64_t n, int32_t* head, int32_t* e,
                        int32_t* nxt, int32_t* belong, double* len)
{
    if (!c) { set_error("dpr_place_exact_run: bad argument"); return DPR_ERR_ARG; }
    // The fast schedule (small subtrees on all CUs + top tree in LDS) gives the reference's lim[] whenever the reference's
    // depths are the tree's depths.  They stop being that only if the default tuple (slot 0, pendant length 2) wins an argmin
    // (updateTreeStructure's swap, src/placement.cu:236-239); the run is then repeated with the literal level-by-depth
    // schedule, the only one that reproduces what the reference computes from there on.
    c->exact.literal = std::getenv("DPR_EXACT_LITERAL") != nullptr;
    int rc = place_exact_attempt(c, source, dist_type, k, n, head, e, nxt, belong, len);
    if (rc != DPR_OK || c->exact.literal) return rc;
    bool quirk = false;
    if (int rq = exact_quirk(c->exact, c->stream, &quirk)) return rq;
    if (!quirk) return DPR_OK;
    c->exact.literal = true;
    rc = place_exact_attempt(c, source, dist_type, k, n, head, e, nxt, belong, len);
    return rc;
}

int dpr_get_exact_state(dpr_ctx* c, int32_t* rev, int32_t* dep)
{
    if (!c || !c->exact.dep || !c->place.rev) { set_error("dpr_get_exact_state: no exact placement state"); return DPR_ERR_STATE; }
    DPR_HIP(hipStreamSynchronize(c->stream));   // the plain copies below run on the null stream, which does not wait for c->stream
    const int64_t n = c->place.N;
    if (rev) DPR_HIP(hipMemcpy(rev, c->place.rev, sizeof(int32_t) * (size_t)(8 * n), hipMemcpyDeviceToHost));
    if (dep) DPR_HIP(hipMemcpy(dep, c->exact.dep, sizeof(int32_t) * (size_t)(2 * n), hipMemcpyDeviceToHost));
    return DPR_OK;
}

// ---- divide-and-conquer mode ------------------------------------------------------------------------
// one dpr_dc_run: what its three steps share.  Everything is released when the run ends (the stream is idle by then on success;
// hipFree waits otherwise), nothing earlier: the budget of the cluster trees is read from the free memory as it stands then.
struct DcRun {
    dpr_ctx* c;
    int source, dist_type, flags;
    int64_t n, B;
    bool real;                       // ranks: RCCL ranks of dpr_comm_init, or -- validation on one GPU -- DPR_DC_VIRTUAL_RANKS(w) emulated in turn
    int W;
    ScopedEvent ev[4];               // backbone | assignment | cluster trees |
    DevBuf<int32_t> d_cl;
    DevBuf<uint64_t> snap_old, snap_acc;
    DcTable tab;
    std::vector<int32_t> h_cl;       // cluster of every tip, -1 for the backbone
    ~DcRun() { dc_table_free(tab); }
};

// the arrays a cluster tree changes, as 64-bit words, each with its offset in a snapshot of all of them
struct DcArr { void* cur; int64_t words, off; };
static std::array<DcArr, 9> dc_arrays(const DcRun& r)
{
    const PlaceBuffers& p = r.c->place;
    const int64_t n = r.n;
    std::array<DcArr, 9> arrs{ { { p.head, n, 0 }, { p.e, 4 * n, 0 }, { p.nxt, 4 * n, 0 }, { p.belong, 4 * n, 0 }, { p.rev, 4 * n, 0 },
                                 { p.len, 8 * n, 0 }, { p.cid, 20 * n, 0 }, { p.cdis, 40 * n, 0 }, { r.c->place_trace, 3 * n, 0 } } };
    for (size_t i = 1; i < arrs.size(); ++i) arrs[i].off = arrs[i - 1].off + arrs[i - 1].words;
    return arrs;
}

// backbone tree: tips [0, B) (findBackboneTreeDC)
static int dc_backbone(DcRun& r)
{
    dpr_ctx* c = r.c;
    DPR_HIP(hipEventRecord(r.ev[0], c->stream));
    if (int rc = place_range(c, r.source, r.dist_type, 2, r.B)) return rc;
    DPR_HIP(hipEventRecord(r.ev[1], c->stream));
    return DPR_OK;
}

// cluster assignment of tips [B, n) (findClustersDC).  Multi-GPU: the backbone is built identically on every rank (same inputs,
// deterministic kernels); the queries are independent, so each rank assigns a contiguous share and the ids are summed (zeros
// elsewhere) over RCCL.
static int dc_assign_queries(DcRun& r)
{
    dpr_ctx* c = r.c;
    const int64_t n = r.n, B = r.B;
    const RowSource src{ c, r.source, r.dist_type };
    if (int rc = dc_table_build(c->place, B, r.tab, c->stream)) return rc;
    const int64_t ts[4] = { r.tab.nv, r.tab.nch, r.tab.max_entries, r.tab.max_leaves };     // (the table is freed with the run)
    std::copy(ts, ts + 4, c->dc_table_stats);
    const int64_t Q = query_batch(B, n - B);
    DevBuf<double> dT;      // (released before the budget of the cluster trees is read)
    DPR_HIP(dT.alloc((size_t)(B * Q)));
    DPR_HIP(r.d_cl.alloc((size_t)(n + 1)));
    DPR_HIP(hipMemsetAsync(r.d_cl, 0, sizeof(int32_t) * (size_t)(n + 1), c->stream));
    // the reference's aligned-input kernel never writes the distance to backbone tip B-1
    // (src/divide_and_conquer/msa.cu:331 `idx>=ed-st`) and scans the 0.0 of a fresh allocation
    const bool skip_last = r.source == DPR_SRC_MSA && !(r.flags & DPR_DC_EXACT_LAST);
    auto assign = [&]() -> int {
        for (int v = 0; v < r.W; ++v) {
            if (r.real && v != c->rank) continue;     // virtual ranks: every share is processed here, one after the other
            int64_t q0 = 0, q1 = 0;
            dc_query_share(n, B, v, r.W, &q0, &q1);
            for (int64_t i0 = q0; i0 < q1; i0 += Q) {
                const int64_t nr = q1 - i0 < Q ? q1 - i0 : Q;
                if (int rc = src.fill(i0, nr, dT, Q, B, c->stream, true)) return rc;
                if (skip_last) DPR_HIP(hipMemsetAsync(dT + (B - 1) * Q, 0, sizeof(double) * (size_t)Q, c->stream));
                if (int rc = dc_assign(r.tab, dT, Q, (int)nr, r.d_cl + i0, c->stream)) return rc;
            }
        }
        if (r.real) {
            if (int rc = comm_all_reduce_sum(c, r.d_cl, (size_t)n, kNcclInt32, c->stream)) return rc;
        }
        DPR_HIP(hipMemcpyAsync(r.h_cl.data(), r.d_cl, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        DPR_HIP(hipEventRecord(r.ev[2], c->stream));
        return DPR_OK;
    };
    const int rc = assign();
    const hipError_t se = hipStreamSynchronize(c->stream);      // (the stream is idle before the scope releases dT)
    if (rc) return rc;
    DPR_HIP(se);
    for (int64_t t = 0; t < B; ++t) r.h_cl[(size_t)t] = -1;
    return DPR_OK;
}

// cluster trees (findClusterTreeDC).  Multi-GPU: clusters are dealt to the ranks; an array element is changed by at most one
// rank, so the states are merged as old + sum of (new - old) (dc_delta_*).
static int dc_cluster_trees(DcRun& r)
{
    dpr_ctx* c = r.c;
    const int64_t n = r.n;
    size_t free_b = 0, total_b = 0;
    DPR_HIP(hipMemGetInfo(&free_b, &total_b));
    size_t budget = free_b / 2;
    if (const char* env = std::getenv("DPR_DC_BUDGET_MB")) budget = (size_t)std::atoll(env) << 20;
    auto phase = [&](int v) -> int {
        return dc_cluster_phase(c->place, r.h_cl.data(), n, r.B, r.source, r.dist_type, &c->msa, &c->mash, c->place_trace, budget, &c->dc_stats, v, r.W, c->stream);
    };
    if (r.W == 1) return phase(0);
    const bool real = r.real;
    auto copy_words = [&](void* dst, const void* src, int64_t words) -> int {
        DPR_HIP(hipMemcpyAsync(dst, src, sizeof(uint64_t) * (size_t)words, hipMemcpyDeviceToDevice, c->stream));
        return DPR_OK;
    };
    const auto arrs = dc_arrays(r);
    const int64_t tot = arrs.back().off + arrs.back().words;
    DPR_HIP(r.snap_old.alloc((size_t)tot));
    if (!real) { DPR_HIP(r.snap_acc.alloc((size_t)tot)); DPR_HIP(hipMemsetAsync(r.snap_acc, 0, sizeof(uint64_t) * (size_t)tot, c->stream)); }
    uint64_t* old = r.snap_old;
    uint64_t* acc = r.snap_acc;
    for (const DcArr& a : arrs) { if (int rc = copy_words(old + a.off, a.cur, a.words)) return rc; }
    if (budget > sizeof(uint64_t) * (size_t)tot * 2) budget -= sizeof(uint64_t) * (size_t)tot * 2;
    for (int v = 0; v < r.W; ++v) {
        if (real && v != c->rank) continue;
        if (!real && v > 0) {                // next virtual rank starts from the backbone state again
            for (const DcArr& a : arrs) { if (int rc = copy_words(a.cur, old + a.off, a.words)) return rc; }
        }
        if (int rc = phase(v)) return rc;
        for (const DcArr& a : arrs) {
            if (int rc = dc_delta_sub(a.cur, old + a.off, a.words, c->stream)) return rc;
            if (!real) { if (int rc = dc_delta_add(acc + a.off, a.cur, a.words, c->stream)) return rc; }
        }
    }
    for (const DcArr& a : arrs) {
        if (int rc = real ? comm_all_reduce_sum(c, a.cur, (size_t)a.words, kNcclUint64, c->stream) : copy_words(a.cur, acc + a.off, a.words)) return rc;
        if (int rc = dc_delta_add(a.cur, old + a.off, a.words, c->stream)) return rc;
    }
    return DPR_OK;
}

int dpr_dc_run(dpr_ctx* c, int source, int dist_type, int k, int64_t n, int64_t backbone, int flags, int32_t* head,
               int32_t* e, int32_t* nxt, int32_t* belong, double* len, int32_t* cluster_id)
{
    if (!c || !head || !e || !nxt || !belong || !len || n < 4) { set_error("dpr_dc_run: bad argument"); return DPR_ERR_ARG; }
    if (backbone < 3 || backbone >= n) { set_error("dpr_dc_run: backbone size must be in [3, n)"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    if (source != DPR_SRC_MSA && source != DPR_SRC_MASH) {
        // src/divide_and_conquer/placement_close_k.cu:969-972
        set_error("dpr_dc_run: input must be unaligned or aligned sequences for the clustering based approach");
        return DPR_ERR_ARG;
    }
    if (int rc = check_source(c, "dpr_dc_run", source, k, n)) return rc;
    if (source == DPR_SRC_MSA && c->msa.aa) { set_error("dpr_dc_run: divide-and-conquer is not available for a protein alignment (nucleotide alignments only)"); return DPR_ERR_ARG; }
    if (int rc = rebuild_place(c, n, backbone)) return rc;
    if (int rc = reset_place_trace(c, n)) return rc;
    const int vw = (flags >> 8) & 0xff;
    DcRun r{ c, source, dist_type, flags, n, backbone, comm_real(c), 1 };
    r.W = r.real ? c->world : (vw > 1 ? vw : 1);
    r.h_cl.assign((size_t)n, -1);
    for (auto& x : r.ev) DPR_HIP(hipEventCreate(x.put()));
    if (int rc = dc_backbone(r)) return rc;
    if (int rc = dc_assign_queries(r)) return rc;
    if (int rc = dc_cluster_trees(r)) return rc;
    DPR_HIP(hipEventRecord(r.ev[3], c->stream));
    if (int rc = copy_adjacency(c, n, false, head, e, nxt, belong, len)) return rc;
    DPR_HIP(hipStreamSynchronize(c->stream));
    float ms = 0;
    DPR_HIP(hipEventElapsedTime(&ms, r.ev[0], r.ev[1])); c->dc_ms[0] = ms;
    DPR_HIP(hipEventElapsedTime(&ms, r.ev[1], r.ev[2])); c->dc_ms[1] = ms;
    DPR_HIP(hipEventElapsedTime(&ms, r.ev[2], r.ev[3])); c->dc_ms[2] = ms;
    c->nj_ms = c->dc_ms[0] + c->dc_ms[1] + c->dc_ms[2];
    if (cluster_id) std::copy(r.h_cl.begin(), r.h_cl.end(), cluster_id);
    return DPR_OK;
}

int dpr_dc_query_share(int64_t n, int64_t backbone, int rank, int world, int64_t* q0, int64_t* q1)
{
    if (!q0 || !q1 || world < 1 || rank < 0 || rank >= world || backbone < 0 || backbone > n) { set_error("dpr_dc_query_share: bad argument"); return DPR_ERR_ARG; }
    dc_query_share(n, backbone, rank, world, q0, q1);
    return DPR_OK;
}

int dpr_dc_deal_clusters(const int64_t* sizes_desc, int64_t count, int world, int32_t* owner)
{
    if (!sizes_desc || !owner || count < 0 || world < 1) { set_error("dpr_dc_deal_clusters: bad argument"); return DPR_ERR_ARG; }
    dc_deal_clusters(sizes_desc, count, world, owner);
    return DPR_OK;
}

int dpr_get_dc_stats(dpr_ctx* c, int64_t* counts5, double* phase_ms3)
{
    if (!c) { set_error("dpr_get_dc_stats: null ctx"); return DPR_ERR_ARG; }
    if (counts5) {
        counts5[0] = c->dc_stats.clusters; counts5[1] = c->dc_stats.max_cluster; counts5[2] = c->dc_stats.pairs;
        counts5[3] = c->dc_stats.groups; counts5[4] = c->dc_stats.jobs;
    }
    if (phase_ms3) for (int i = 0; i < 3; ++i) phase_ms3[i] = c->dc_ms[i];
    return DPR_OK;
}

int dpr_get_dc_table_stats(dpr_ctx* c, int64_t out4[4])
{
    if (!c || !out4) { set_error("dpr_get_dc_table_stats: null argument"); return DPR_ERR_ARG; }
    std::copy(c->dc_table_stats, c->dc_table_stats + 4, out4);
    return DPR_OK;
}

// Per placed tip of the last placement run: how many slots its closest-list walk reached (updateClosestNodes,
// src/placement_close_k.cu:86-124, serial there) beyond the two rounds the split applies in registers; negative = -(reached + 1):
// the walk started at the new leaf because a node of degree > 3 lies behind the split edge (imported backbones only).  One
// wavefront takes 64 queue entries per round trip, so a tip's update launch grows with this number: it is what the outliers of
// place_update_kernel is made of.  The four-tip launch (place_update_multi_kernel) has a second kind: its speculative block
// minima stand except where an earlier tip of the same launch changed an input (the "dirty" slots: the walks' slots and their
// reverses); when those outgrow the set (2 048), or more than 128 blocks must be re-scanned, the launch evaluates EVERY slot itself --
// milliseconds on a 500 000-tip tree.  stats6 (optional): tips whose walk left the 2 048-entry LDS queue, largest walk, sum over
// the tips, tips that took the degree > 3 walk, tips of four-tip launches that fell back to the full evaluation because the dirty
// set overflowed, ... because too many blocks had to be re-scanned.
int dpr_get_place_walks(dpr_ctx* c, int32_t* reached /* n, or NULL */, int64_t* stats4)
{
    if (!c || !c->place.bfs_cnt) { set_error("dpr_get_place_walks: no placement state"); return DPR_ERR_STATE; }
    DPR_HIP(hipStreamSynchronize(c->stream));
    const int64_t n = c->place.N;
    std::vector<int32_t> h((size_t)n);
    DPR_HIP(hipMemcpy(h.data(), c->place.bfs_cnt, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    if (reached) std::copy(h.begin(), h.end(), reached);
    if (stats4) {
        stats4[0] = stats4[1] = stats4[2] = stats4[3] = 0;
        int32_t misc[4] = { 0, 0, 0, 0 };
        DPR_HIP(hipMemcpy(misc, c->place.misc, sizeof misc, hipMemcpyDeviceToHost));
        stats4[4] = misc[2]; stats4[5] = misc[3];
        for (int32_t v : h) {
            const int64_t r = v < 0 ? -(int64_t)v - 1 : v;
            if (r > 2048) ++stats4[0];
            if (r > stats4[1]) stats4[1] = r;
            stats4[2] += r;
            if (v < 0) ++stats4[3];
        }
    }
    return DPR_OK;
}

int dpr_get_place_state(dpr_ctx* c, int32_t* cid, double* cdis, double* trace)
{
    if (!c || !c->place.cid) { set_error("dpr_get_place_state: no placement state"); return DPR_ERR_STATE; }
    DPR_HIP(hipStreamSynchronize(c->stream));   // the plain copies below run on the null stream, which does not wait for c->stream
    const int64_t n = c->place.N;
    if (cid) DPR_HIP(hipMemcpy(cid, c->place.cid, sizeof(int32_t) * (size_t)(40 * n), hipMemcpyDeviceToHost));
    if (cdis) DPR_HIP(hipMemcpy(cdis, c->place.cdis, sizeof(double) * (size_t)(40 * n), hipMemcpyDeviceToHost));
    if (trace) DPR_HIP(hipMemcpy(trace, c->place_trace, sizeof(double) * (size_t)(3 * n), hipMemcpyDeviceToHost));
    return DPR_OK;
}

// ---- independent placement on a fixed backbone (pfix.hip) -------------------------------------------------------------
int dpr_place_fixed_set(dpr_ctx* c, int64_t m, int64_t n, const int32_t* head, const int32_t* e, const int32_t* nxt,
                        const int32_t* belong, const double* len)
{
    if (!c || !head || !e || !nxt || !belong || !len || m < 3 || m >= n) { set_error("dpr_place_fixed_set: bad argument (3 <= m < n)"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    if (int rc = check_backbone_slots("dpr_place_fixed_set", m, e, belong)) return rc;
    if (int rc = rebuild_place(c, n)) return rc;
    // (the arrays are only read: host -> device)
    if (int rc = copy_adjacency(c, n, true, const_cast<int32_t*>(head), const_cast<int32_t*>(e), const_cast<int32_t*>(nxt),
                                const_cast<int32_t*>(belong), const_cast<double*>(len))) return rc;
    if (int rc = place_import_backbone(c->place, m, c->stream)) return rc;
    if (int rc = pfix_set(c->pfix, c->place, m, c->stream)) return rc;
    DPR_HIP(hipStreamSynchronize(c->stream));
    return DPR_OK;
}

int dpr_ctx_set_place_fixed_batch(dpr_ctx* c, int64_t queries)
{
    if (!c || queries < 0 || queries > 65536) { set_error("dpr_ctx_set_place_fixed_batch: 0 (the rule of dpr_dc_run) .. 65536 queries"); return DPR_ERR_ARG; }
    c->pfix.batch = queries;
    return DPR_OK;
}

int dpr_place_fixed_run(dpr_ctx* c, int source, int dist_type, int k, int32_t* slot, double* frac, double* add)
{
    if (!c || !slot || !frac || !add) { set_error("dpr_place_fixed_run: bad argument"); return DPR_ERR_ARG; }
    PlaceFixed& f = c->pfix;
    if (!f.valid) { set_error("dpr_place_fixed_run: call dpr_place_fixed_set first (a placement run since then has replaced the backbone)"); return DPR_ERR_STATE; }
    DPR_HIP(hipSetDevice(c->device));
    if (source != DPR_SRC_MSA && source != DPR_SRC_MASH) { set_error("dpr_place_fixed_run: input must be unaligned or aligned sequences"); return DPR_ERR_ARG; }
    const int64_t n = f.n, m = f.m, nq = n - m;
    if (int rc = check_source(c, "dpr_place_fixed_run", source, k, n)) return rc;
    const bool real = comm_real(c);
    const int W = real ? c->world : 1, rank = real ? c->rank : 0;
    // contiguous query shares as dpr_dc_query_share: rank r takes [m + r * share, m + (r + 1) * share) below n, and its results are
    // segment r of the all-gather
    const int64_t share = ((nq + W - 1) / W + 255) / 256 * 256;
    int64_t q0 = 0, q1 = 0;
    dc_query_share(n, m, rank, W, &q0, &q1);
    const int64_t Q = f.batch > 0 ? f.batch : query_batch(m, nq);      // (dpr_ctx_set_place_fixed_batch overrides the rule)
    if ((size_t)(m * Q) > f.dT_cap) {
        if (f.dT) { (void)hipFree(f.dT); f.dT = nullptr; f.dT_cap = 0; }
        DPR_HIP(hipMalloc(&f.dT, sizeof(double) * (size_t)(m * Q)));
        f.dT_cap = (size_t)(m * Q);
    }
    if ((size_t)(share * W) > f.out_cap) {
        void* old[] = { f.slot, f.frac, f.add };
        for (void* q : old)
            if (q) (void)hipFree(q);
        f.slot = nullptr; f.frac = nullptr; f.add = nullptr; f.out_cap = 0;
        DPR_HIP(hipMalloc(&f.slot, sizeof(int32_t) * (size_t)(share * W)));
        DPR_HIP(hipMalloc(&f.frac, sizeof(double) * (size_t)(share * W)));
        DPR_HIP(hipMalloc(&f.add, sizeof(double) * (size_t)(share * W)));
        f.out_cap = (size_t)(share * W);
    }
    const bool carry = std::getenv("DPR_PFIX_CARRY") != nullptr && std::atoi(std::getenv("DPR_PFIX_CARRY")) != 0;
    const RowSource src{ c, source, dist_type };
    std::vector<ScopedEvent> ev;      // per batch: start, distances done, placed
    auto mark = [&]() -> int { ev.emplace_back(); DPR_HIP(hipEventCreate(ev.back().put())); DPR_HIP(hipEventRecord(ev.back(), c->stream)); return DPR_OK; };
    auto run = [&]() -> int {
        if (real) {      // (segments of other ranks' trailing, unused entries are gathered too: defined)
            DPR_HIP(hipMemsetAsync(f.slot + rank * share, 0xff, sizeof(int32_t) * (size_t)share, c->stream));
            DPR_HIP(hipMemsetAsync(f.frac + rank * share, 0, sizeof(double) * (size_t)share, c->stream));
            DPR_HIP(hipMemsetAsync(f.add + rank * share, 0, sizeof(double) * (size_t)share, c->stream));
        }
        for (int64_t i0 = q0; i0 < q1; i0 += Q) {
            const int64_t nr = q1 - i0 < Q ? q1 - i0 : Q, o = i0 - m;
            if (int rc = mark()) return rc;
            if (int rc = src.fill(i0, nr, f.dT, Q, m, c->stream, true)) return rc;
            if (int rc = mark()) return rc;
            if (int rc = pfix_place(f, f.dT, Q, (int)nr, f.slot + o, f.frac + o, f.add + o, carry, c->stream)) return rc;
            if (int rc = mark()) return rc;
        }
        if (real) {
            if (int rc = comm_all_gather(c, f.slot + rank * share, f.slot, sizeof(int32_t) * (size_t)share, c->stream)) return rc;
            if (int rc = comm_all_gather(c, f.frac + rank * share, f.frac, sizeof(double) * (size_t)share, c->stream)) return rc;
            if (int rc = comm_all_gather(c, f.add + rank * share, f.add, sizeof(double) * (size_t)share, c->stream)) return rc;
        }
        DPR_HIP(hipMemcpyAsync(slot, f.slot, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
        DPR_HIP(hipMemcpyAsync(frac, f.frac, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
        DPR_HIP(hipMemcpyAsync(add, f.add, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, c->stream));
        return DPR_OK;
    };
    const int rc = run();
    const hipError_t se = hipStreamSynchronize(c->stream);      // (the stream is idle before the events are released)
    if (rc) return rc;
    DPR_HIP(se);
    c->pfix_ms[0] = c->pfix_ms[1] = 0;
    for (size_t i = 0; i + 2 < ev.size(); i += 3)
        for (int k2 = 0; k2 < 2; ++k2) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[i + (size_t)k2], ev[i + (size_t)k2 + 1]) == hipSuccess) c->pfix_ms[k2] += ms;
        }
    return DPR_OK;
}

int dpr_get_place_fixed_timing(dpr_ctx* c, double* dist_ms, double* scan_ms)
{
    if (!c) { set_error("dpr_get_place_fixed_timing: null ctx"); return DPR_ERR_ARG; }
    if (dist_ms) *dist_ms = c->pfix_ms[0];
    if (scan_ms) *scan_ms = c->pfix_ms[1];
    return DPR_OK;
}

}  // extern "C"
