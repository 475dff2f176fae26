// C ABI of the pairs within a distance threshold and their clusters (include/dipper_hip.h, dpr_pairs_*): the stream of row blocks over
// the context's uploaded source.  Kernels in pairs.hip, the host restatement in pairs_host.hpp.  The n x n matrix is never allocated: a
// block of rows is computed by the source's row provider (the one placement batches use), filtered, copied back and forgotten.
#include "pairs_host.hpp"
#include "place_rows.hpp"

using namespace dpr;

namespace {

// device memory of the stream, counted as it is allocated (dpr_pairs_stats reports the peak)
template <class T> int pairs_dev_alloc(PairsBuffers& p, DevBuf<T>& buf, size_t count)
{
    DPR_HIP(buf.alloc(count ? count : 1));
    p.dev_bytes += (int64_t)(sizeof(T) * (count ? count : 1));
    if (p.dev_bytes > p.peak_bytes) p.peak_bytes = p.dev_bytes;
    return DPR_OK;
}

int pairs_pinned(PinnedBuf& buf, size_t bytes)
{
    DPR_HIP(hipHostMalloc(buf.put(), bytes ? bytes : 1, hipHostMallocDefault));
    return DPR_OK;
}

// room for `total` pairs of a block on both sides; what is there is dropped first (a block's pairs do not outlive the next call)
int pairs_reserve(PairsBuffers& p, int64_t total)
{
    if (total <= p.cap) return DPR_OK;
    int64_t cap = p.cap > 0 ? p.cap : 4096;
    while (cap < total) cap *= 2;
    const int64_t most = p.block_rows * (p.n - 1);      // no block holds more
    if (cap > most) cap = most;
    p.dev_bytes -= p.cap * 16;
    p.pi.reset(); p.pj.reset(); p.pd.reset();
    p.hi.reset(); p.hj.reset(); p.hd.reset();
    p.cap = 0;
    if (int rc = pairs_dev_alloc(p, p.pi, (size_t)cap)) return rc;
    if (int rc = pairs_dev_alloc(p, p.pj, (size_t)cap)) return rc;
    if (int rc = pairs_dev_alloc(p, p.pd, (size_t)cap)) return rc;
    if (int rc = pairs_pinned(p.hi, sizeof(int32_t) * (size_t)cap)) return rc;
    if (int rc = pairs_pinned(p.hj, sizeof(int32_t) * (size_t)cap)) return rc;
    if (int rc = pairs_pinned(p.hd, sizeof(double) * (size_t)cap)) return rc;
    p.cap = cap;
    return DPR_OK;
}

}  // namespace

extern "C" {

int dpr_pairs_begin(dpr_ctx* c, int source, int dist_type, int k, double threshold, int64_t block_rows)
{
    if (!c) { set_error("dpr_pairs_begin: null ctx"); return DPR_ERR_ARG; }
    if (!pairs::threshold_ok(threshold)) { set_error("dpr_pairs_begin: the threshold must be a finite number >= 0"); return DPR_ERR_ARG; }
    if (block_rows < 0) { set_error("dpr_pairs_begin: block_rows must be >= 0"); return DPR_ERR_ARG; }
    if (c->world > 1 || c->vworld > 0) { set_error("dpr_pairs_begin: one rank only"); return DPR_ERR_ARG; }
    int64_t n = 0;
    if (source == DPR_SRC_MSA) {
        if (!c->msa.planes) { set_error("dpr_pairs_begin: call dpr_set_msa first"); return DPR_ERR_STATE; }
        n = c->msa.n;
    } else if (source == DPR_SRC_MATRIX) {
        if (!c->packed_lower) { set_error("dpr_pairs_begin: call dpr_set_matrix_lower first"); return DPR_ERR_STATE; }
        n = c->n_input;
    } else if (source == DPR_SRC_MASH) {
        if (!c->mash.sketches) { set_error("dpr_pairs_begin: call dpr_set_reads and dpr_sketch first"); return DPR_ERR_STATE; }
        if (k != c->mash.k) { set_error("dpr_pairs_begin: k differs from the sketch k"); return DPR_ERR_ARG; }
        n = c->mash.n;
    } else {
        set_error("dpr_pairs_begin: source not available");
        return DPR_ERR_ARG;
    }
    DPR_HIP(hipSetDevice(c->device));
    c->pairs.reset(new PairsBuffers());
    PairsBuffers& p = *c->pairs;
    p.source = source; p.dist_type = dist_type; p.threshold = threshold; p.n = n;
    p.ld = (n + 15) / 16 * 16;
    // block_rows 0: the rows whose block fits kPairsBlockBytes, in whole tiles of 64 rows where there are that many
    int64_t rows = block_rows > 0 ? block_rows : kPairsBlockBytes / ((int64_t)sizeof(double) * p.ld);
    if (block_rows == 0 && rows > 64) rows -= rows % 64;
    rows = rows < 1 ? 1 : rows > kPairsMaxRows ? kPairsMaxRows : rows;
    p.block_rows = rows < n ? rows : n;
    int rc = DPR_OK;
    if (source != DPR_SRC_MATRIX) rc = pairs_dev_alloc(p, p.block, (size_t)(p.block_rows * p.ld));
    if (rc == DPR_OK) rc = pairs_dev_alloc(p, p.cnt, (size_t)(p.block_rows + 1));
    if (rc == DPR_OK) rc = pairs_dev_alloc(p, p.parent, (size_t)n);
    if (rc == DPR_OK) rc = pairs_pinned(p.htotal, sizeof(int64_t));
    if (rc == DPR_OK) rc = pairs_parent_init(p.parent, n, c->stream);
    if (rc == DPR_OK && hipStreamSynchronize(c->stream) != hipSuccess) rc = hip_fail(hipGetLastError(), "dpr_pairs_begin: parents");
    if (rc != DPR_OK) c->pairs.reset();
    return rc;
}

int dpr_pairs_next(dpr_ctx* c, const int32_t** i, const int32_t** j, const double** d, int64_t* count, int64_t* rows_done)
{
    if (!c || !i || !j || !d || !count || !rows_done) { set_error("dpr_pairs_next: null argument"); return DPR_ERR_ARG; }
    if (!c->pairs) { set_error("dpr_pairs_next: call dpr_pairs_begin first"); return DPR_ERR_STATE; }
    PairsBuffers& p = *c->pairs;
    *i = nullptr; *j = nullptr; *d = nullptr; *count = 0; *rows_done = p.next_row;
    if (p.next_row >= p.n) { p.ended = true; return DPR_OK; }
    DPR_HIP(hipSetDevice(c->device));
    const int64_t r0 = p.next_row, nr = p.n - r0 < p.block_rows ? p.n - r0 : p.block_rows;
    const bool packed = p.source == DPR_SRC_MATRIX;
    const double* rows = packed ? c->packed_lower : p.block.get();
    hipStream_t s = c->stream;
    EventPairs tm;      // the provider; count + scan; write + hook; the copies
    const RowSource src{ c, p.source, p.dist_type };
    if (int rc = tm.begin(s)) return rc;
    if (int rc = src.fill(r0, nr, p.block, p.ld, r0 + nr, s)) return rc;
    if (int rc = tm.end(s)) return rc;
    if (int rc = tm.begin(s)) return rc;
    if (int rc = pairs_count_scan(rows, p.ld, packed, r0, nr, p.threshold, p.cnt, s)) return rc;
    if (int rc = tm.end(s)) return rc;
    DPR_HIP(hipMemcpyAsync(p.htotal.get(), p.cnt.get() + nr, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    DPR_HIP(hipStreamSynchronize(s));
    const int64_t total = *static_cast<const int64_t*>(p.htotal.get());
    if (total < 0 || total > nr * (p.n - 1)) { set_error("dpr_pairs_next: a block's pair count is out of range"); return DPR_ERR_STATE; }
    if (int rc = pairs_reserve(p, total)) return rc;
    if (int rc = tm.begin(s)) return rc;
    if (int rc = pairs_write_hook(rows, p.ld, packed, r0, nr, p.threshold, p.cnt, total, p.pi, p.pj, p.pd, p.parent, p.n, s)) return rc;
    if (int rc = tm.end(s)) return rc;
    if (int rc = tm.begin(s)) return rc;
    if (total > 0) {
        DPR_HIP(hipMemcpyAsync(p.hi.get(), p.pi.get(), sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, s));
        DPR_HIP(hipMemcpyAsync(p.hj.get(), p.pj.get(), sizeof(int32_t) * (size_t)total, hipMemcpyDeviceToHost, s));
        DPR_HIP(hipMemcpyAsync(p.hd.get(), p.pd.get(), sizeof(double) * (size_t)total, hipMemcpyDeviceToHost, s));
    }
    if (int rc = tm.end(s)) return rc;
    DPR_HIP(hipStreamSynchronize(s));
    p.dist_ms += tm.ms(0) > 0 ? tm.ms(0) : 0;
    p.filter_ms += (tm.ms(1) > 0 ? tm.ms(1) : 0) + (tm.ms(2) > 0 ? tm.ms(2) : 0);
    p.copy_ms += tm.ms(3) > 0 ? tm.ms(3) : 0;
    p.next_row = r0 + nr;
    ++p.blocks;
    p.pairs += total;
    if (total > 0) { *i = static_cast<const int32_t*>(p.hi.get()); *j = static_cast<const int32_t*>(p.hj.get()); *d = static_cast<const double*>(p.hd.get()); }
    *count = total;
    *rows_done = p.next_row;
    if (total == 0 && p.next_row >= p.n) p.ended = true;      // (the last block held nothing: this call is the end of the stream)
    return DPR_OK;
}

int dpr_pairs_labels(dpr_ctx* c, int32_t* label)
{
    if (!c || !label) { set_error("dpr_pairs_labels: null argument"); return DPR_ERR_ARG; }
    if (!c->pairs) { set_error("dpr_pairs_labels: call dpr_pairs_begin first"); return DPR_ERR_STATE; }
    PairsBuffers& p = *c->pairs;
    if (p.next_row < p.n) { set_error("dpr_pairs_labels: the stream has not ended (dpr_pairs_next until rows_done == n)"); return DPR_ERR_STATE; }
    DPR_HIP(hipSetDevice(c->device));
    DevBuf<int32_t> out;
    DPR_HIP(out.alloc((size_t)p.n));
    if (p.dev_bytes + 4 * p.n > p.peak_bytes) p.peak_bytes = p.dev_bytes + 4 * p.n;
    if (int rc = pairs_flatten(p.parent, out, p.n, c->stream)) return rc;
    DPR_HIP(hipMemcpyAsync(label, out, sizeof(int32_t) * (size_t)p.n, hipMemcpyDeviceToHost, c->stream));
    DPR_HIP(hipStreamSynchronize(c->stream));
    int64_t sum[3] = { 0, 0, 0 };
    if (pairs::summarize(label, p.n, sum, nullptr)) { set_error("dpr_pairs_labels: a label is not the smallest index of its component"); return DPR_ERR_STATE; }
    p.comps = sum[0]; p.largest = sum[1]; p.singletons = sum[2];
    p.ended = true; p.labelled = true;
    return DPR_OK;
}

int dpr_pairs_stats(dpr_ctx* c, int64_t out[6])
{
    if (!c || !out) { set_error("dpr_pairs_stats: null argument"); return DPR_ERR_ARG; }
    if (!c->pairs) { set_error("dpr_pairs_stats: call dpr_pairs_begin first"); return DPR_ERR_STATE; }
    const PairsBuffers& p = *c->pairs;
    out[0] = p.blocks; out[1] = p.pairs; out[2] = p.comps; out[3] = p.largest; out[4] = p.singletons; out[5] = p.peak_bytes;
    return DPR_OK;
}

int dpr_get_pairs_info(dpr_ctx* c, double ms[3], int64_t shape[2])
{
    if (!c) { set_error("dpr_get_pairs_info: null ctx"); return DPR_ERR_ARG; }
    if (!c->pairs) { set_error("dpr_get_pairs_info: call dpr_pairs_begin first"); return DPR_ERR_STATE; }
    if (ms) { ms[0] = c->pairs->dist_ms; ms[1] = c->pairs->filter_ms; ms[2] = c->pairs->copy_ms; }
    if (shape) { shape[0] = c->pairs->block_rows; shape[1] = c->pairs->n; }
    return DPR_OK;
}

int dpr_pairs_end(dpr_ctx* c)
{
    if (!c) { set_error("dpr_pairs_end: null ctx"); return DPR_ERR_ARG; }
    if (!c->pairs) return DPR_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->pairs.reset();
    return DPR_OK;
}

int dpr_pairs_within_host(const double* lower_rows, int64_t n, double threshold, int32_t* i, int32_t* j, double* d, int64_t cap, int64_t* count,
                          int32_t* label)
{
    if (pairs::within_host(lower_rows, n, threshold, i, j, d, cap, count, label)) { set_error("dpr_pairs_within_host: bad argument"); return DPR_ERR_ARG; }
    return DPR_OK;
}

int dpr_pairs_summary_host(const int32_t* label, int64_t n, int64_t out3[3], int32_t* rank)
{
    if (pairs::summarize(label, n, out3, rank)) { set_error("dpr_pairs_summary_host: bad argument, or labels that are not component minima"); return DPR_ERR_ARG; }
    return DPR_OK;
}

}  // extern "C"
