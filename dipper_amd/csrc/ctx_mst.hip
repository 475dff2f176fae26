// C ABI of the minimum spanning forest of the distances (include/dipper_hip.h, dpr_mst_*): Boruvka rounds over the context's uploaded
// source.  Kernels in mst.hip, the host restatement, the order of the edges and their check in mst_host.hpp.  The n x n matrix is never
// allocated: in every round each block of full rows is computed by the source's row provider (the one the streams of pairs and of
// neighbours use), or expanded from the packed triangle, reduced to one minimum a row and forgotten.
#include "mst_host.hpp"
#include "pairs_host.hpp"
#include "place_rows.hpp"

using namespace dpr;

namespace {

// device memory of a call, counted as it is allocated (dpr_mst_stats reports the sum: everything lives until the call returns)
template <class T> int mst_dev_alloc(MstState& m, DevBuf<T>& buf, size_t count)
{
    DPR_HIP(buf.alloc(count ? count : 1));
    m.peak_bytes += (int64_t)(sizeof(T) * (count ? count : 1));
    return DPR_OK;
}

int mst_rounds_bound(int64_t n)      // ceil(log2 n) + 1: the components with an edge at least halve every round, then one round finds nothing
{
    int lg = 0;
    while (((int64_t)1 << lg) < n) ++lg;
    return lg + 1;
}

}  // namespace

extern "C" {

int dpr_mst_run(dpr_ctx* c, int source, int dist_type, int k, int64_t block_rows, int32_t* ei, int32_t* ej, double* ed, int64_t* edges,
                int32_t* label)
{
    if (!c || !ei || !ej || !ed || !edges || !label) { set_error("dpr_mst_run: null argument"); return DPR_ERR_ARG; }
    if (block_rows < 0) { set_error("dpr_mst_run: block_rows must be >= 0"); return DPR_ERR_ARG; }
    if (c->world > 1 || c->vworld > 0) { set_error("dpr_mst_run: one rank only"); return DPR_ERR_ARG; }
    int64_t n = 0;
    if (source == DPR_SRC_MSA) {
        if (!c->msa.planes) { set_error("dpr_mst_run: call dpr_set_msa first"); return DPR_ERR_STATE; }
        n = c->msa.n;
    } else if (source == DPR_SRC_MATRIX) {
        if (!c->packed_lower) { set_error("dpr_mst_run: call dpr_set_matrix_lower first"); return DPR_ERR_STATE; }
        n = c->n_input;
    } else if (source == DPR_SRC_MASH) {
        if (!c->mash.sketches) { set_error("dpr_mst_run: call dpr_set_reads and dpr_sketch first"); return DPR_ERR_STATE; }
        if (k != c->mash.k) { set_error("dpr_mst_run: k differs from the sketch k"); return DPR_ERR_ARG; }
        n = c->mash.n;
    } else {
        set_error("dpr_mst_run: source not available");
        return DPR_ERR_ARG;
    }
    if (n < 2) { set_error("dpr_mst_run: at least two sequences"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    c->mst.reset();
    MstState m;
    m.n = n;
    const int64_t ld = (n + 15) / 16 * 16;
    // block_rows 0: the rule of the streams of pairs and of neighbours -- the rows whose block fits kPairsBlockBytes, in whole tiles of 64
    int64_t rows = block_rows > 0 ? block_rows : kPairsBlockBytes / ((int64_t)sizeof(double) * ld);
    if (block_rows == 0 && rows > 64) rows -= rows % 64;
    rows = rows < 1 ? 1 : rows > kPairsMaxRows ? kPairsMaxRows : rows;
    m.block_rows = rows < n ? rows : n;
    const int64_t cap = n - 1;
    DevBuf<double> block, rdist, ded;
    DevBuf<int32_t> dlabel, rcol, dei, dej;
    DevBuf<unsigned long long> rkey, ckey, cedge, dcount;
    PinnedBuf hcount;
    int rc = mst_dev_alloc(m, block, (size_t)(m.block_rows * ld));
    if (rc == DPR_OK) rc = mst_dev_alloc(m, dlabel, (size_t)ld);      // (ld entries: the walk loads labels in pairs, as it loads columns)
    if (rc == DPR_OK) rc = mst_dev_alloc(m, rkey, (size_t)n);
    if (rc == DPR_OK) rc = mst_dev_alloc(m, rcol, (size_t)n);
    if (rc == DPR_OK) rc = mst_dev_alloc(m, rdist, (size_t)n);
    if (rc == DPR_OK) rc = mst_dev_alloc(m, ckey, (size_t)n);
    if (rc == DPR_OK) rc = mst_dev_alloc(m, cedge, (size_t)n);
    if (rc == DPR_OK) rc = mst_dev_alloc(m, dei, (size_t)cap);
    if (rc == DPR_OK) rc = mst_dev_alloc(m, dej, (size_t)cap);
    if (rc == DPR_OK) rc = mst_dev_alloc(m, ded, (size_t)cap);
    if (rc == DPR_OK) rc = mst_dev_alloc(m, dcount, 1);
    if (rc != DPR_OK) return rc;
    DPR_HIP(hipHostMalloc(hcount.put(), sizeof(unsigned long long), hipHostMallocDefault));
    hipStream_t s = c->stream;
    const RowSource src{ c, source, dist_type };
    DPR_HIP(hipMemsetAsync(dcount, 0, sizeof(unsigned long long), s));
    if (int r2 = pairs_parent_init(dlabel, n, s)) return r2;
    const int bound = mst_rounds_bound(n);
    int64_t total = 0, comps = n;
    for (;;) {
        if (m.rounds >= bound) { set_error("dpr_mst_run: more rounds than ceil(log2 n) + 1"); return DPR_ERR_STATE; }
        EventPairs tm;      // per block: the provider or the expansion, the row minimum; then the component work and the copy
        int64_t nblocks = 0;
        for (int64_t r0 = 0; r0 < n; r0 += m.block_rows, ++nblocks) {
            const int64_t nr = n - r0 < m.block_rows ? n - r0 : m.block_rows;
            if (int r2 = tm.begin(s)) return r2;
            if (source == DPR_SRC_MATRIX) {
                if (int r2 = nearest_expand_packed(c->packed_lower, n, r0, nr, block, ld, s)) return r2;
            } else {
                if (int r2 = src.fill(r0, nr, block, ld, n, s, false, false, true)) return r2;
            }
            if (int r2 = tm.end(s)) return r2;
            if (int r2 = tm.begin(s)) return r2;
            if (int r2 = mst_row_min(block, ld, r0, nr, n, dlabel, rkey, rcol, rdist, s)) return r2;
            if (int r2 = tm.end(s)) return r2;
        }
        if (int r2 = tm.begin(s)) return r2;
        if (int r2 = mst_component_min_emit(dlabel, rkey, rcol, rdist, n, ckey, cedge, dei, dej, ded, cap, dcount, s)) return r2;
        DPR_HIP(hipMemcpyAsync(hcount.get(), dcount.get(), sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        if (int r2 = tm.end(s)) return r2;
        DPR_HIP(hipStreamSynchronize(s));      // the one synchronisation of a round
        const int64_t count = (int64_t)*static_cast<const unsigned long long*>(hcount.get());
        for (int64_t b = 0; b < nblocks; ++b) {
            m.dist_ms += tm.ms((size_t)(2 * b)) > 0 ? tm.ms((size_t)(2 * b)) : 0;
            m.rowmin_ms += tm.ms((size_t)(2 * b + 1)) > 0 ? tm.ms((size_t)(2 * b + 1)) : 0;
        }
        m.round_ms += tm.ms((size_t)(2 * nblocks)) > 0 ? tm.ms((size_t)(2 * nblocks)) : 0;
        ++m.rounds;
        m.blocks += nblocks;
        m.rows_walked += n;
        if (count < total || count > cap) { set_error("dpr_mst_run: more edges than a forest holds"); return DPR_ERR_STATE; }
        const int64_t emitted = count - total;
        if (emitted > 0) {
            if (int r2 = pairs_hook(dei.get() + total, dej.get() + total, emitted, dlabel, n, s)) return r2;
            if (int r2 = pairs_flatten(dlabel, dlabel, n, s)) return r2;
        }
        total = count;
        comps -= emitted;
        if (emitted == 0 || comps <= 1) break;
    }
    std::vector<int32_t> hi((size_t)cap), hj((size_t)cap), hl((size_t)n), want((size_t)n);
    std::vector<double> hd((size_t)cap);
    if (total > 0) {
        DPR_HIP(hipMemcpyAsync(hi.data(), dei.get(), sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, s));
        DPR_HIP(hipMemcpyAsync(hj.data(), dej.get(), sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, s));
        DPR_HIP(hipMemcpyAsync(hd.data(), ded.get(), sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, s));
    }
    DPR_HIP(hipMemcpyAsync(hl.data(), dlabel.get(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, s));
    DPR_HIP(hipStreamSynchronize(s));
    // the contract's order; replaying it must never meet two tips already joined, must give the device's labels, and E = n - C
    int64_t sum[3] = { 0, 0, 0 };
    if (mst::order_and_label(n, hi.data(), hj.data(), hd.data(), total, want.data()) || want != hl || pairs::summarize(hl.data(), n, sum, nullptr) ||
        total != n - sum[0]) {
        set_error("dpr_mst_run: the edges found are no spanning forest of the components (a source whose D_rc and D_cr differ?)");
        return DPR_ERR_STATE;
    }
    m.edges = total; m.comps = sum[0]; m.largest = sum[1]; m.singletons = sum[2];
    std::copy(hi.begin(), hi.begin() + total, ei);
    std::copy(hj.begin(), hj.begin() + total, ej);
    std::copy(hd.begin(), hd.begin() + total, ed);
    std::copy(hl.begin(), hl.end(), label);
    *edges = total;
    c->mst.reset(new MstState(m));
    return DPR_OK;
}

int dpr_mst_stats(dpr_ctx* c, int64_t out[8])
{
    if (!c || !out) { set_error("dpr_mst_stats: null argument"); return DPR_ERR_ARG; }
    if (!c->mst) { set_error("dpr_mst_stats: call dpr_mst_run first"); return DPR_ERR_STATE; }
    const MstState& m = *c->mst;
    out[0] = m.rounds; out[1] = m.blocks; out[2] = m.edges; out[3] = m.comps; out[4] = m.largest; out[5] = m.singletons;
    out[6] = m.peak_bytes; out[7] = m.rows_walked;
    return DPR_OK;
}

int dpr_get_mst_info(dpr_ctx* c, double ms[3], int64_t shape[2])
{
    if (!c) { set_error("dpr_get_mst_info: null ctx"); return DPR_ERR_ARG; }
    if (!c->mst) { set_error("dpr_get_mst_info: call dpr_mst_run first"); return DPR_ERR_STATE; }
    if (ms) { ms[0] = c->mst->dist_ms; ms[1] = c->mst->rowmin_ms; ms[2] = c->mst->round_ms; }
    if (shape) { shape[0] = c->mst->block_rows; shape[1] = c->mst->n; }
    return DPR_OK;
}

int dpr_mst_host(const double* lower_rows, int64_t n, int32_t* ei, int32_t* ej, double* ed, int64_t* edges, int32_t* label)
{
    if (mst::mst_host(lower_rows, n, ei, ej, ed, edges, label)) { set_error("dpr_mst_host: bad argument (n >= 2, no null pointer)"); return DPR_ERR_ARG; }
    return DPR_OK;
}

int dpr_mst_dendrogram_host(int64_t n, const int32_t* ei, const int32_t* ej, const double* ed, int64_t edges, int32_t* merge_x,
                            int32_t* merge_y, double* height)
{
    if (mst::dendrogram_host(n, ei, ej, ed, edges, merge_x, merge_y, height)) {
        set_error("dpr_mst_dendrogram_host: bad argument, or edges that do not connect the tips (n - 1 edges of a spanning tree)");
        return DPR_ERR_ARG;
    }
    return DPR_OK;
}

}  // extern "C"
