// Distance rows for the tree builders of ctx_place.hip: the row source, the timers of a k-closest placement run and its
// two-buffer row pipeline.  Which batch is produced beside the tree kernels is not decided here (place_policy.hpp).
#pragma once
#include "ctx_internal.hpp"

namespace dpr {

// distance rows of a source: MSA and Mash rows are computed into a buffer, the packed triangle is read in place
struct RowSource {
    dpr_ctx* c;
    int source, dist_type;
    // rows [i0, i0 + nr) x columns [0, ncols) into out (row stride ld; transposed: column stride ld); beside: tree kernels of
    // another stream run during these launches (the only place that sets MashBuffers::share_chip); full: a row's columns beyond its own
    // index are wanted too (the MSA provider writes every column below ncols anyway)
    int fill(int64_t i0, int64_t nr, double* out, int64_t ld, int64_t ncols, hipStream_t st, bool transposed = false, bool beside = false,
             bool full = false) const
    {
        if (nr <= 0) return DPR_OK;
        if (source == DPR_SRC_MSA) return msa_dist_block_rows(c->msa, i0, nr, 0, 0, ncols, dist_type, out, ld, st, transposed);
        if (source != DPR_SRC_MASH) return DPR_OK;
        c->mash.share_chip = beside;
        const int rc = mash_dist_rows(c->mash, i0, nr, 0, 0, full, ncols, out, ld, st, transposed);
        c->mash.share_chip = false;
        return rc;
    }
    // row i of a buffer that starts at row i0 (row stride ld), or of the packed triangle
    const double* row_ptr(int64_t i, int64_t i0, const double* rows, int64_t ld) const
    {
        return source == DPR_SRC_MATRIX ? c->packed_lower + i * (i - 1) / 2 : rows + (i - i0) * ld;
    }
};

// event pairs of one kind, owned for the run: begin() ... end() around work on a stream
struct EventPairs {
    std::vector<ScopedEvent> ev;      // pair k: ev[2k], ev[2k + 1]
    int begin(hipStream_t s)
    {
        for (int i = 0; i < 2; ++i) { ev.emplace_back(); DPR_HIP(hipEventCreate(ev.back().put())); }
        DPR_HIP(hipEventRecord(ev[ev.size() - 2], s));
        return DPR_OK;
    }
    int end(hipStream_t s) { DPR_HIP(hipEventRecord(ev.back(), s)); return DPR_OK; }
    double ms(size_t k) const      // negative: not (both) recorded
    {
        float t = 0;
        return 2 * k + 1 < ev.size() && hipEventElapsedTime(&t, ev[2 * k], ev[2 * k + 1]) == hipSuccess ? (double)t : -1.0;
    }
    double total() const
    {
        double tot = 0;
        for (size_t k = 0; 2 * k + 1 < ev.size(); ++k) { const double t = ms(k); if (t > 0) tot += t; }
        return tot;
    }
};

// The reference reports the distance and the tree part of a placement run separately (src/placement_close_k.cu:852-853,985-986).
// A batch produced on the main stream: a pair around it (dist).  A batch produced beside the tree kernels: its own interval
// overlaps the tree work in wall time (and stretches while it shares the chip) -- kept as `busy`; what counts as distance time is
// the time the tree stream actually WAITED for it (a pair around the wait, dist again), so distance + tree = the run's wall time.
// Every batch has one pair in dist and one in tree, at its own index; the packed triangle has no distance part and no timers.
struct PlaceTimers {
    EventPairs dist, busy, tree;
    // the host waits for batch k's tree kernels; what the overlap policy observes of that batch
    int wait_batch(size_t k, double* tree_ms, double* dist_ms) const
    {
        DPR_HIP(hipEventSynchronize(tree.ev[2 * k + 1]));
        *tree_ms = tree.ms(k);
        *dist_ms = dist.ms(k);
        return DPR_OK;
    }
    // both streams idle: the figures of dpr_get_place_timing / dpr_get_place_overlap
    void finish(dpr_ctx* c) const { c->place_dist_ms = dist.total(); c->place_dist_busy_ms = busy.total(); }
};

// The rows of a run's batches.  Batch k lives in buffer k & 1 when batches may be produced beside the tree kernels (`two`: a
// second buffer and the context's low-priority stream2), else in the one buffer.  A producer waits for the batch that last read
// the buffer it overwrites; on its first use of the second buffer it waits for everything enqueued so far.
struct RowPipeline {
    dpr_ctx* c;
    RowSource src;
    PlaceTimers t;                            // every event pair of the run
    bool two = false, sharded = false;
    int W = 1;
    int64_t per = 0, ldb = 0;                 // rows per rank and batch; row stride
    DevBuf<double> buf[2];
    std::vector<ScopedEvent> order;           // owns the filled / consumed events below
    hipEvent_t filled[2] = { nullptr, nullptr }, consumed[2] = { nullptr, nullptr };

    RowPipeline(dpr_ctx* ctx, int source, int dist_type) : c(ctx), src{ ctx, source, dist_type } {}
    bool timed() const { return src.source != DPR_SRC_MATRIX; }
    double* rows(size_t k) const { return buf[two ? k & 1 : 0]; }

    int init(int64_t R, int64_t last, bool overlap_allowed)
    {
        two = overlap_allowed;
        ldb = (last + 15) / 16 * 16;
        // Multi-GPU (dpr_comm_init done, inputs replicated): the distance rows of a batch do not depend on the placements, so
        // every rank computes R / world of them and one all-gather per batch completes the block; the tree kernels then run
        // identically on every rank (deterministic), so no tree state is exchanged.
        sharded = comm_real(c) && src.source != DPR_SRC_MATRIX;
        W = sharded ? c->world : 1;
        per = (R + W - 1) / W;
        if (src.source != DPR_SRC_MATRIX) {
            DPR_HIP(buf[0].alloc((size_t)(per * W * ldb)));
            if (two) {
                const hipError_t me = buf[1].alloc((size_t)(per * W * ldb));
                if (me != hipSuccess) return hip_fail(me, "hipMalloc(second row buffer)");
            }
        }
        if (two && !c->stream2) {
            // lowest priority: the distance kernels fill the chip, the tree kernels of the current batch (one wavefront or a few
            // blocks each, on the context's stream) must not queue behind them
            int least = 0, greatest = 0;
            DPR_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
            DPR_HIP(hipStreamCreateWithPriority(&c->stream2, hipStreamNonBlocking, least));
        }
        return DPR_OK;
    }
    int mark(hipEvent_t* e, hipStream_t s)      // a fresh ordering event, recorded on s
    {
        order.emplace_back();
        DPR_HIP(hipEventCreateWithFlags(order.back().put(), hipEventDisableTiming));
        *e = order.back();
        DPR_HIP(hipEventRecord(*e, s));
        return DPR_OK;
    }
    // rows [i0, i0 + nr) x columns [0, i0 + nr): this rank's share and the batch's all-gather
    int fill(int64_t i0, int64_t nr, double* out, hipStream_t s, bool beside)
    {
        if (!sharded) return src.fill(i0, nr, out, ldb, i0 + nr, s, false, beside);
        const int64_t a = (int64_t)c->rank * per, b = a + per < nr ? a + per : nr;
        if (int rc = src.fill(i0 + a, b - a, out + a * ldb, ldb, i0 + nr, s, false, beside)) return rc;
        return comm_all_gather(c, out + a * ldb, out, sizeof(double) * (size_t)(per * ldb), s);
    }
    int produce(size_t k, int64_t i0, int64_t nr, bool beside)
    {
        hipStream_t s = beside ? c->stream2 : c->stream;
        EventPairs& tm = beside ? t.busy : t.dist;
        if (timed()) { if (int rc = tm.begin(s)) return rc; }
        const int rc = fill(i0, nr, rows(k), s, beside);
        if (timed()) { if (int rc2 = tm.end(s)) return rc2; }
        return rc;
    }
    // batch k on stream2, beside whatever the main stream runs from here on
    int produce_beside(size_t k, int64_t i0, int64_t nr)
    {
        const int b = (int)(k & 1);
        if (consumed[b]) DPR_HIP(hipStreamWaitEvent(c->stream2, consumed[b], 0));
        else {      // (first use of that buffer by the second stream: everything enqueued so far may still read it)
            hipEvent_t e = nullptr;
            if (int rc = mark(&e, c->stream)) return rc;
            DPR_HIP(hipStreamWaitEvent(c->stream2, e, 0));
        }
        if (int rc = produce(k, i0, nr, true)) return rc;
        return mark(&filled[b], c->stream2);
    }
    // batch k for the tree stream: produced on it now, at full chip (a buffer's last reader ran on this stream: ordered), or --
    // produced beside its predecessor -- the tree stream waits for the producer, and that wait is the batch's distance time
    int make_available(size_t k, int64_t i0, int64_t nr, bool ahead)
    {
        if (!ahead) return produce(k, i0, nr, false);
        if (int rc = t.dist.begin(c->stream)) return rc;
        DPR_HIP(hipStreamWaitEvent(c->stream, filled[k & 1], 0));
        return t.dist.end(c->stream);
    }
    int mark_consumed(size_t k) { return two ? mark(&consumed[k & 1], c->stream) : DPR_OK; }
    // both streams are done with the row buffers (and the events) before the scope releases them
    void drain() const
    {
        if (!buf[0] && !buf[1]) return;
        (void)hipStreamSynchronize(c->stream);
        if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    }
};

}  // namespace dpr
