// C ABI of each sequence's K nearest neighbours (include/dipper_hip.h, dpr_nearest_*): the stream of row blocks over the context's
// uploaded source.  Kernels in nearest.hip, the host restatement in nearest_host.hpp.  The n x n matrix is never allocated: a block of
// full rows is computed by the source's row provider (the one placement batches and the stream of pairs use), or expanded from the
// packed triangle, selected from, copied back and forgotten.
#include "nearest_host.hpp"
#include "place_rows.hpp"

using namespace dpr;

static_assert(nearest::kNearestMaxK == dpr::kNearestMaxK && DPR_NEAREST_MAX_K == dpr::kNearestMaxK, "one largest K");

namespace {

// device memory of the stream, counted as it is allocated (dpr_nearest_stats reports the peak)
template <class T> int nearest_dev_alloc(NearestBuffers& b, DevBuf<T>& buf, size_t count)
{
    DPR_HIP(buf.alloc(count ? count : 1));
    b.dev_bytes += (int64_t)(sizeof(T) * (count ? count : 1));
    if (b.dev_bytes > b.peak_bytes) b.peak_bytes = b.dev_bytes;
    return DPR_OK;
}

int nearest_pinned(PinnedBuf& buf, size_t bytes)
{
    DPR_HIP(hipHostMalloc(buf.put(), bytes ? bytes : 1, hipHostMallocDefault));
    return DPR_OK;
}

}  // namespace

extern "C" {

int dpr_nearest_begin(dpr_ctx* c, int source, int dist_type, int k, int K, int64_t block_rows)
{
    if (!c) { set_error("dpr_nearest_begin: null ctx"); return DPR_ERR_ARG; }
    if (K < 1 || K > kNearestMaxK) { set_error("dpr_nearest_begin: K must be in [1, 256]"); return DPR_ERR_ARG; }
    if (block_rows < 0) { set_error("dpr_nearest_begin: block_rows must be >= 0"); return DPR_ERR_ARG; }
    if (c->world > 1 || c->vworld > 0) { set_error("dpr_nearest_begin: one rank only"); return DPR_ERR_ARG; }
    int64_t n = 0;
    if (source == DPR_SRC_MSA) {
        if (!c->msa.planes) { set_error("dpr_nearest_begin: call dpr_set_msa first"); return DPR_ERR_STATE; }
        n = c->msa.n;
    } else if (source == DPR_SRC_MATRIX) {
        if (!c->packed_lower) { set_error("dpr_nearest_begin: call dpr_set_matrix_lower first"); return DPR_ERR_STATE; }
        n = c->n_input;
    } else if (source == DPR_SRC_MASH) {
        if (!c->mash.sketches) { set_error("dpr_nearest_begin: call dpr_set_reads and dpr_sketch first"); return DPR_ERR_STATE; }
        if (k != c->mash.k) { set_error("dpr_nearest_begin: k differs from the sketch k"); return DPR_ERR_ARG; }
        n = c->mash.n;
    } else {
        set_error("dpr_nearest_begin: source not available");
        return DPR_ERR_ARG;
    }
    if (n < 2) { set_error("dpr_nearest_begin: at least two sequences"); return DPR_ERR_ARG; }
    DPR_HIP(hipSetDevice(c->device));
    c->nearest.reset(new NearestBuffers());
    NearestBuffers& b = *c->nearest;
    b.source = source; b.dist_type = dist_type; b.K = K; b.n = n;
    b.ld = (n + 15) / 16 * 16;
    // block_rows 0: the rule of the stream of pairs -- the rows whose block fits kPairsBlockBytes, in whole tiles of 64 rows
    int64_t rows = block_rows > 0 ? block_rows : kPairsBlockBytes / ((int64_t)sizeof(double) * b.ld);
    if (block_rows == 0 && rows > 64) rows -= rows % 64;
    rows = rows < 1 ? 1 : rows > kPairsMaxRows ? kPairsMaxRows : rows;
    b.block_rows = rows < n ? rows : n;
    const size_t places = (size_t)(b.block_rows * K);
    int rc = nearest_dev_alloc(b, b.block, (size_t)(b.block_rows * b.ld));
    if (rc == DPR_OK) rc = nearest_dev_alloc(b, b.oj, places);
    if (rc == DPR_OK) rc = nearest_dev_alloc(b, b.od, places);
    if (rc == DPR_OK) rc = nearest_dev_alloc(b, b.ocnt, (size_t)b.block_rows);
    if (rc == DPR_OK) rc = nearest_dev_alloc(b, b.oflush, (size_t)b.block_rows);
    if (rc == DPR_OK) rc = nearest_pinned(b.hj, sizeof(int32_t) * places);
    if (rc == DPR_OK) rc = nearest_pinned(b.hd, sizeof(double) * places);
    if (rc == DPR_OK) rc = nearest_pinned(b.hcnt, sizeof(int32_t) * (size_t)b.block_rows);
    if (rc == DPR_OK) rc = nearest_pinned(b.hflush, sizeof(int32_t) * (size_t)b.block_rows);
    if (rc != DPR_OK) c->nearest.reset();
    return rc;
}

int dpr_nearest_next(dpr_ctx* c, const int32_t** j, const double** d, const int32_t** cnt, int64_t* row0, int64_t* rows)
{
    if (!c || !j || !d || !cnt || !row0 || !rows) { set_error("dpr_nearest_next: null argument"); return DPR_ERR_ARG; }
    if (!c->nearest) { set_error("dpr_nearest_next: call dpr_nearest_begin first"); return DPR_ERR_STATE; }
    NearestBuffers& b = *c->nearest;
    *j = nullptr; *d = nullptr; *cnt = nullptr; *row0 = b.next_row; *rows = 0;
    if (b.next_row >= b.n) return DPR_OK;
    DPR_HIP(hipSetDevice(c->device));
    const int64_t r0 = b.next_row, nr = b.n - r0 < b.block_rows ? b.n - r0 : b.block_rows;
    const size_t places = (size_t)(nr * b.K);
    hipStream_t s = c->stream;
    EventPairs tm;      // the provider or the expansion; the select; the copies
    const RowSource src{ c, b.source, b.dist_type };
    if (int rc = tm.begin(s)) return rc;
    if (b.source == DPR_SRC_MATRIX) {
        if (int rc = nearest_expand_packed(c->packed_lower, b.n, r0, nr, b.block, b.ld, s)) return rc;
    } else {
        if (int rc = src.fill(r0, nr, b.block, b.ld, b.n, s, false, false, true)) return rc;
    }
    if (int rc = tm.end(s)) return rc;
    if (int rc = tm.begin(s)) return rc;
    if (int rc = nearest_select(b.block, b.ld, r0, nr, b.n, b.K, b.oj, b.od, b.ocnt, b.oflush, s)) return rc;
    if (int rc = tm.end(s)) return rc;
    if (int rc = tm.begin(s)) return rc;
    DPR_HIP(hipMemcpyAsync(b.hj.get(), b.oj.get(), sizeof(int32_t) * places, hipMemcpyDeviceToHost, s));
    DPR_HIP(hipMemcpyAsync(b.hd.get(), b.od.get(), sizeof(double) * places, hipMemcpyDeviceToHost, s));
    DPR_HIP(hipMemcpyAsync(b.hcnt.get(), b.ocnt.get(), sizeof(int32_t) * (size_t)nr, hipMemcpyDeviceToHost, s));
    DPR_HIP(hipMemcpyAsync(b.hflush.get(), b.oflush.get(), sizeof(int32_t) * (size_t)nr, hipMemcpyDeviceToHost, s));
    if (int rc = tm.end(s)) return rc;
    DPR_HIP(hipStreamSynchronize(s));
    const int32_t* hc = static_cast<const int32_t*>(b.hcnt.get());
    const int32_t* hf = static_cast<const int32_t*>(b.hflush.get());
    int64_t found = 0, fewer = 0, none = 0, flushes = 0;
    for (int64_t t = 0; t < nr; ++t) {
        if (hc[t] < 0 || hc[t] > b.K || hc[t] > b.n - 1) { set_error("dpr_nearest_next: a row's count is out of range"); return DPR_ERR_STATE; }
        found += hc[t]; fewer += hc[t] < b.K; none += hc[t] == 0; flushes += hf[t];
    }
    b.dist_ms += tm.ms(0) > 0 ? tm.ms(0) : 0;
    b.select_ms += tm.ms(1) > 0 ? tm.ms(1) : 0;
    b.copy_ms += tm.ms(2) > 0 ? tm.ms(2) : 0;
    b.next_row = r0 + nr;
    ++b.blocks;
    b.neighbours += found; b.fewer += fewer; b.none += none; b.flushes += flushes;
    *j = static_cast<const int32_t*>(b.hj.get());
    *d = static_cast<const double*>(b.hd.get());
    *cnt = hc;
    *row0 = r0;
    *rows = nr;
    return DPR_OK;
}

int dpr_nearest_stats(dpr_ctx* c, int64_t out[6])
{
    if (!c || !out) { set_error("dpr_nearest_stats: null argument"); return DPR_ERR_ARG; }
    if (!c->nearest) { set_error("dpr_nearest_stats: call dpr_nearest_begin first"); return DPR_ERR_STATE; }
    const NearestBuffers& b = *c->nearest;
    out[0] = b.blocks; out[1] = b.neighbours; out[2] = b.fewer; out[3] = b.none; out[4] = b.flushes; out[5] = b.peak_bytes;
    return DPR_OK;
}

int dpr_get_nearest_info(dpr_ctx* c, double ms[3], int64_t shape[2])
{
    if (!c) { set_error("dpr_get_nearest_info: null ctx"); return DPR_ERR_ARG; }
    if (!c->nearest) { set_error("dpr_get_nearest_info: call dpr_nearest_begin first"); return DPR_ERR_STATE; }
    if (ms) { ms[0] = c->nearest->dist_ms; ms[1] = c->nearest->select_ms; ms[2] = c->nearest->copy_ms; }
    if (shape) { shape[0] = c->nearest->block_rows; shape[1] = c->nearest->n; }
    return DPR_OK;
}

int dpr_nearest_end(dpr_ctx* c)
{
    if (!c) { set_error("dpr_nearest_end: null ctx"); return DPR_ERR_ARG; }
    if (!c->nearest) return DPR_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    c->nearest.reset();
    return DPR_OK;
}

int dpr_nearest_host(const double* lower_rows, int64_t n, int K, int32_t* j, double* d, int32_t* cnt)
{
    if (nearest::nearest_host(lower_rows, n, K, j, d, cnt)) { set_error("dpr_nearest_host: bad argument (n >= 2, 1 <= K <= 256, no null pointer)"); return DPR_ERR_ARG; }
    return DPR_OK;
}

}  // extern "C"
