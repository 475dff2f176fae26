"""ctypes binding of include/dipper_hip.h.  Thin: every method is one C-ABI call (plus numpy
buffer plumbing).  There is no Python or CPU fallback -- if the library or the GPU is missing the
call raises."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

SRC_MSA, SRC_MASH, SRC_MATRIX = 1, 2, 3
DIST_UNCORRECTED, DIST_JC = 1, 2
DIST_POISSON, DIST_KIMURA = 7, 8     # protein alignments only (Dipper.set_msa_aa)
DIST_TN93, DIST_LOGDET, DIST_PARALINEAR = 9, 10, 11     # nucleotide alignments only (Dipper.set_msa)

c_i32p = C.POINTER(C.c_int32)
c_i64p = C.POINTER(C.c_int64)
c_u64p = C.POINTER(C.c_uint64)
c_f64p = C.POINTER(C.c_double)


class DipperError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"dipper_hip error {code}: {msg}")
        self.code = code


def library_path():
    # (DPR_LIB: another build of the library -- kernel-variant experiments under profiles/)
    return os.environ.get("DPR_LIB") or os.path.join(_HERE, "libdipper_hip.so")


def load_library():
    """Loads libdipper_hip.so (built in-tree by __graft_entry__.build()).  Raises if absent."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = C.CDLL(path)
    L.dpr_last_error.restype = C.c_char_p
    L.dpr_abi_version.restype = C.c_int
    L.dpr_pack4.argtypes = [C.c_char_p, C.c_uint64, c_u64p]
    L.dpr_pack2.argtypes = [C.c_char_p, C.c_uint64, c_u64p]
    L.dpr_pack_aa.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.c_uint8)]
    L.dpr_njr_owner.argtypes = [C.c_int64, C.c_int]
    L.dpr_njr_local_row.argtypes = [C.c_int64, C.c_int]
    L.dpr_njr_local_row.restype = C.c_int64
    L.dpr_njr_global_pos.argtypes = [C.c_int64, C.c_int, C.c_int]
    L.dpr_njr_global_pos.restype = C.c_int64
    L.dpr_njr_rows_cap.argtypes = [C.c_int64, C.c_int]
    L.dpr_njr_rows_cap.restype = C.c_int64
    L.dpr_shard_owner.argtypes = [C.c_int64, C.c_int]
    L.dpr_shard_local_row.argtypes = [C.c_int64, C.c_int]
    L.dpr_shard_local_row.restype = C.c_int64
    L.dpr_shard_rows.argtypes = [C.c_int64, C.c_int, C.c_int]
    L.dpr_shard_rows.restype = C.c_int64
    L.dpr_shard_global_row.argtypes = [C.c_int64, C.c_int, C.c_int]
    L.dpr_shard_global_row.restype = C.c_int64
    L.dpr_record_reduce.argtypes = [C.c_void_p, C.c_int]
    L.dpr_nj_key.argtypes = [C.c_int64, C.c_int64, C.c_int64]
    L.dpr_nj_key.restype = C.c_uint64
    L.dpr_create.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.dpr_create_virtual.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.c_int]
    L.dpr_destroy.argtypes = [C.c_void_p]
    L.dpr_device_name.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.dpr_comm_unique_id.argtypes = [C.c_void_p]
    L.dpr_comm_init.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    L.dpr_comm_selftest.argtypes = [C.c_void_p]
    L.dpr_comm_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dpr_comm_init_local.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.dpr_comm_init_shared.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_uint64, C.c_int]
    L.dpr_comm_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64)]
    L.dpr_shared_abort.argtypes = [C.c_void_p]
    L.dpr_shared_failed.argtypes = [C.c_void_p]
    L.dpr_shared_barrier.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint32), C.c_int]
    L.dpr_shared_gather.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_uint32), C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    L.dpr_peer_export.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    L.dpr_peer_attach.argtypes = [C.c_void_p, C.c_void_p]
    L.dpr_ctx_set_nj_exchange.argtypes = [C.c_void_p, C.c_int]
    L.dpr_get_nj_exchange_info.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int]
    L.dpr_ctx_set_poll_limit_ms.argtypes = [C.c_void_p, C.c_int]
    L.dpr_ctx_set_nj_adaptive.argtypes = [C.c_void_p, C.c_int]
    L.dpr_get_nj_adaptive_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dpr_scan_tune.argtypes = [C.c_int, C.c_int, C.c_int]
    L.dpr_set_nj_mode.argtypes = [C.c_int]
    L.dpr_set_nj_multi_plan.argtypes = [C.c_int]
    L.dpr_nj_is_unit_sharded.argtypes = [C.c_void_p]
    L.dpr_get_nj_multi_info.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.dpr_ctx_set_nj_mode.argtypes = [C.c_void_p, C.c_int]
    L.dpr_ctx_set_nj_multi_plan.argtypes = [C.c_void_p, C.c_int]
    L.dpr_ctx_set_nj_virtual_shards.argtypes = [C.c_void_p, C.c_int]
    L.dpr_ctx_set_nj_kernel_timing.argtypes = [C.c_void_p, C.c_int]
    L.dpr_ctx_set_nj_variant.argtypes = [C.c_void_p, C.c_int]
    L.dpr_get_nj_lambda.argtypes = [C.c_void_p, c_f64p, C.POINTER(C.c_int64)]
    L.dpr_nj_variant_host.argtypes = [C.c_int, c_f64p, C.c_int64, C.c_int64, c_i32p, c_i32p, c_f64p, c_f64p, c_f64p, c_f64p]
    L.dpr_nj_variant_host.restype = C.c_int64
    L.dpr_get_nj_kernel_timing.argtypes = [C.c_void_p, C.POINTER(C.c_int), c_f64p, C.POINTER(C.c_int64)]
    L.dpr_nj_kernel_name.argtypes = [C.c_int]
    L.dpr_nj_kernel_name.restype = C.c_char_p
    L.dpr_get_place_timing.argtypes = [C.c_void_p, c_f64p, c_f64p]
    L.dpr_get_place_overlap.argtypes = [C.c_void_p, C.POINTER(C.c_int), c_f64p]
    L.dpr_get_place_policy.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dpr_get_prune_stats.argtypes = [C.c_void_p, c_u64p, c_u64p]
    L.dpr_ctx_set_debug_fault.argtypes = [C.c_void_p, C.c_int64, C.c_int]
    L.dpr_get_nj_progress.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dpr_get_njp_shape.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.dpr_bw_probe.argtypes = [C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.dpr_set_msa.argtypes = [C.c_void_p, c_u64p, C.c_int64, C.c_int64]
    L.dpr_set_msa_aa.argtypes = [C.c_void_p, C.POINTER(C.c_uint8), C.c_int64, C.c_int64]
    L.dpr_set_reads.argtypes = [C.c_void_p, c_u64p, c_u64p, c_u64p, C.c_int64]
    L.dpr_set_matrix_lower.argtypes = [C.c_void_p, c_f64p, C.c_int64]
    L.dpr_sketch.argtypes = [C.c_void_p, C.c_int, C.c_int, c_u64p]
    L.dpr_get_mash_index_info.argtypes = [C.c_void_p, c_i64p]
    L.dpr_dist_matrix.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    L.dpr_reserve_nj.argtypes = [C.c_void_p, C.c_int64]
    L.dpr_warm_graphs.argtypes = [C.c_void_p]
    L.dpr_nj_run.argtypes = [C.c_void_p, C.c_int64, c_i32p, c_i32p, c_f64p, c_f64p, c_f64p]
    L.dpr_nj_run.restype = C.c_int64
    L.dpr_argmin_once.argtypes = [C.c_void_p, C.c_int, c_i32p, c_i32p, c_f64p, C.POINTER(C.c_float)]
    L.dpr_n_active.argtypes = [C.c_void_p]
    L.dpr_n_active.restype = C.c_int64
    L.dpr_n_total.argtypes = [C.c_void_p]
    L.dpr_n_total.restype = C.c_int64
    L.dpr_get_matrix_row.argtypes = [C.c_void_p, C.c_int64, c_f64p]
    L.dpr_get_row_sums.argtypes = [C.c_void_p, c_f64p]
    L.dpr_get_msa_counts.argtypes = [C.c_void_p, C.c_int64, c_i32p, c_i32p]
    L.dpr_msa_dist_block.argtypes = [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int, C.c_int, c_f64p, C.c_int, C.POINTER(C.c_float)]
    L.dpr_get_kmer_hashes.argtypes = [C.c_void_p, C.c_int64, C.c_int, c_u64p, c_u64p, c_u64p]
    L.dpr_get_place_state.argtypes = [C.c_void_p, c_i32p, c_f64p, c_f64p]
    L.dpr_get_place_walks.argtypes = [C.c_void_p, c_i32p, C.POINTER(C.c_int64)]
    L.dpr_get_timing.argtypes = [C.c_void_p, c_f64p, c_f64p]
    L.dpr_place_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64,
                                c_i32p, c_i32p, c_i32p, c_i32p, c_f64p]
    L.dpr_place_exact_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                      c_i32p, c_i32p, c_i32p, c_i32p, c_f64p]
    L.dpr_get_exact_state.argtypes = [C.c_void_p, c_i32p, c_i32p]
    L.dpr_dc_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int,
                             c_i32p, c_i32p, c_i32p, c_i32p, c_f64p, c_i32p]
    L.dpr_place_fixed_set.argtypes = [C.c_void_p, C.c_int64, C.c_int64, c_i32p, c_i32p, c_i32p, c_i32p, c_f64p]
    L.dpr_place_fixed_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, c_i32p, c_f64p, c_f64p]
    L.dpr_ctx_set_place_fixed_batch.argtypes = [C.c_void_p, C.c_int64]
    L.dpr_get_place_fixed_timing.argtypes = [C.c_void_p, c_f64p, c_f64p]
    L.dpr_njp_unit_owner.argtypes = [C.c_int64, C.c_int64, C.c_int64, C.c_int]
    L.dpr_place_policy_run.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_int64, c_f64p, c_f64p, C.c_int64, c_i32p]
    L.dpr_nj_plan_resolve.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64, C.c_uint64]
    L.dpr_dc_query_share.argtypes = [C.c_int64, C.c_int64, C.c_int, C.c_int, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.dpr_dc_deal_clusters.argtypes = [C.POINTER(C.c_int64), C.c_int64, C.c_int, c_i32p]
    L.dpr_get_dc_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), c_f64p]
    L.dpr_get_dc_table_stats.argtypes = [C.c_void_p, c_i64p]
    L.dpr_msa_resample.argtypes = [C.c_void_p, C.c_uint64, C.c_int64]
    L.dpr_get_msa_boot_weights.argtypes = [C.c_void_p, c_i32p]
    L.dpr_msa_boot_weights.argtypes = [C.c_uint64, C.c_int64, C.c_int64, c_i32p]
    L.dpr_get_msa_site_coverage.argtypes = [C.c_void_p, c_i32p]
    L.dpr_msa_filter_sites.argtypes = [C.c_void_p, C.c_int]
    L.dpr_msa_filter_sites.restype = C.c_int64
    L.dpr_split_support.argtypes = [C.c_int64, c_i32p, c_i32p, c_i32p, c_i32p, c_i32p]
    L.dpr_comm_sum_i32.argtypes = [C.c_void_p, c_i32p, C.c_int64]
    L.dpr_transfer_support.argtypes = [C.c_void_p, C.c_int64, c_i32p, c_i32p, c_i32p, c_i32p, c_i64p]
    _bme_out = [C.c_int, c_i32p, c_i32p, c_f64p, c_f64p, c_i64p]
    L.dpr_bme_nni.argtypes = [C.c_void_p, C.c_int64, c_i32p, c_i32p] + _bme_out
    L.dpr_bme_nni_host.argtypes = [c_f64p, C.c_int64, c_i32p, c_i32p] + _bme_out
    L.dpr_bme_eval_host.argtypes = [c_f64p, C.c_int64, c_i32p, C.c_int32, c_f64p, c_f64p, c_i32p, c_f64p]
    L.dpr_get_bme_timing.argtypes = [C.c_void_p, c_f64p, c_f64p]
    L.dpr_get_bme_stats.argtypes = [C.c_void_p, c_i64p]
    L.dpr_bme_spr.argtypes = [C.c_void_p, C.c_int64, c_i32p, c_i32p] + _bme_out
    L.dpr_bme_spr_host.argtypes = [c_f64p, C.c_int64, c_i32p, c_i32p] + _bme_out
    L.dpr_bme_spr_eval_host.argtypes = [c_f64p, C.c_int64, c_i32p, C.c_int32, c_f64p, c_i32p, c_i32p, c_f64p]
    L.dpr_bme_spr_gain_host.argtypes = [c_f64p, C.c_int64, c_i32p, C.c_int32, C.c_int64, C.c_int32, c_f64p, c_i32p]
    L.dpr_get_bme_spr_timing.argtypes = [C.c_void_p, c_f64p]
    L.dpr_get_bme_spr_stats.argtypes = [C.c_void_p, c_i64p]
    L.dpr_upgma_run.argtypes = [C.c_void_p, C.c_int, c_i32p, c_i32p, c_f64p]
    L.dpr_upgma_run.restype = C.c_int64
    L.dpr_upgma_host.argtypes = [c_f64p, C.c_int64, C.c_int, c_i32p, c_i32p, c_f64p]
    L.dpr_get_upgma_stats.argtypes = [C.c_void_p, c_i64p]
    L.dpr_get_upgma_timing.argtypes = [C.c_void_p, c_f64p]
    _fit_out = [c_f64p, c_f64p, c_i64p, c_i32p]
    L.dpr_tree_fit.argtypes = [C.c_void_p, C.c_int64, C.c_int64, c_i32p, c_f64p] + _fit_out
    L.dpr_tree_fit_host.argtypes = [c_f64p, C.c_int64, C.c_int64, c_i32p, c_f64p] + _fit_out
    L.dpr_tree_fit_derive.argtypes = [c_f64p]
    L.dpr_tree_patristic_rows.argtypes = [C.c_void_p, C.c_int64, C.c_int64, c_i32p, c_f64p, C.c_int64, C.c_int64, c_f64p]
    L.dpr_tree_from_nj.argtypes = [C.c_int64, c_i32p, c_i32p, c_f64p, c_f64p, C.c_double, c_i32p, c_f64p, c_i64p]
    L.dpr_tree_from_kids.argtypes = [C.c_int64, c_i32p, C.c_int32, c_f64p, c_i32p, c_f64p, c_i64p]
    L.dpr_tree_from_upgma.argtypes = [C.c_int64, c_i32p, c_i32p, c_f64p, c_i32p, c_f64p, c_i64p]
    L.dpr_get_fit_stats.argtypes = [C.c_void_p, c_i64p]
    L.dpr_get_fit_timing.argtypes = [C.c_void_p, c_f64p, c_f64p, c_f64p]
    L.dpr_ctx_set_fit_compare.argtypes = [C.c_void_p, C.c_int]
    L.dpr_transfer_support_host.argtypes = [C.c_int64, c_i32p, c_i32p, c_i32p, c_i32p, c_i64p]
    L.dpr_transfer_taxa.argtypes = [C.c_void_p, C.c_int64, c_i32p, c_i32p, c_i32p, c_i32p, C.c_int, c_i64p, c_i64p, c_i64p]
    L.dpr_transfer_taxa_host.argtypes = [C.c_int64, c_i32p, c_i32p, c_i32p, c_i32p, C.c_int, c_i64p, c_i64p, c_i64p]
    L.dpr_ctx_set_tbe_lds.argtypes = [C.c_void_p, C.c_int64]
    L.dpr_comm_sum_i64.argtypes = [C.c_void_p, c_i64p, C.c_int64]
    L.dpr_pairs_begin.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int64]
    L.dpr_pairs_next.argtypes = [C.c_void_p, C.POINTER(c_i32p), C.POINTER(c_i32p), C.POINTER(c_f64p), c_i64p, c_i64p]
    L.dpr_pairs_labels.argtypes = [C.c_void_p, c_i32p]
    L.dpr_pairs_stats.argtypes = [C.c_void_p, c_i64p]
    L.dpr_pairs_end.argtypes = [C.c_void_p]
    L.dpr_get_pairs_info.argtypes = [C.c_void_p, c_f64p, c_i64p]
    L.dpr_pairs_within_host.argtypes = [c_f64p, C.c_int64, C.c_double, c_i32p, c_i32p, c_f64p, C.c_int64, c_i64p, c_i32p]
    L.dpr_pairs_summary_host.argtypes = [c_i32p, C.c_int64, c_i64p, c_i32p]
    L.dpr_nearest_begin.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64]
    L.dpr_nearest_next.argtypes = [C.c_void_p, C.POINTER(c_i32p), C.POINTER(c_f64p), C.POINTER(c_i32p), c_i64p, c_i64p]
    L.dpr_nearest_stats.argtypes = [C.c_void_p, c_i64p]
    L.dpr_nearest_end.argtypes = [C.c_void_p]
    L.dpr_get_nearest_info.argtypes = [C.c_void_p, c_f64p, c_i64p]
    L.dpr_nearest_host.argtypes = [c_f64p, C.c_int64, C.c_int, c_i32p, c_f64p, c_i32p]
    L.dpr_mst_run.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64, c_i32p, c_i32p, c_f64p, c_i64p, c_i32p]
    L.dpr_mst_stats.argtypes = [C.c_void_p, c_i64p]
    L.dpr_get_mst_info.argtypes = [C.c_void_p, c_f64p, c_i64p]
    L.dpr_mst_host.argtypes = [c_f64p, C.c_int64, c_i32p, c_i32p, c_f64p, c_i64p, c_i32p]
    L.dpr_mst_dendrogram_host.argtypes = [C.c_int64, c_i32p, c_i32p, c_f64p, C.c_int64, c_i32p, c_i32p, c_f64p]
    _LIB = L
    return L


DC_EXACT_LAST = 1
COMM_SHARED_BYTES = 65536
TRANSPORT_AUTO, TRANSPORT_RCCL, TRANSPORT_IPC = 0, 1, 2


class SharedRegion:
    """DPR_COMM_SHARED_BYTES of shared memory for dpr_comm_init_shared, backed by a file under /dev/shm: the process that
    passes create=True makes it (zero-filled) BEFORE the ranks start, the ranks map it by name.  Test / bench plumbing: the
    `dipper` command forks its ranks around an anonymous shared mapping instead."""

    def __init__(self, name, create=False):
        import mmap
        self.path = os.path.join("/dev/shm", name)
        if create:
            with open(self.path, "wb") as f:
                f.write(b"\0" * COMM_SHARED_BYTES)
        self._f = open(self.path, "r+b")
        self._m = mmap.mmap(self._f.fileno(), COMM_SHARED_BYTES)
        self._buf = (C.c_char * COMM_SHARED_BYTES).from_buffer(self._m)
        self.address = C.addressof(self._buf)
        self.size = COMM_SHARED_BYTES

    def abort(self):
        load_library().dpr_shared_abort(self.address)

    def failed(self):
        return bool(load_library().dpr_shared_failed(self.address))

    def barrier(self, world, sense, timeout_ms=10000):
        L = load_library()
        _chk(L, L.dpr_shared_barrier(self.address, world, C.byref(sense), timeout_ms))

    def gather(self, rank, world, sense, mine: bytes, timeout_ms=10000):
        L = load_library()
        out = (C.c_char * (len(mine) * world))()
        _chk(L, L.dpr_shared_gather(self.address, rank, world, C.byref(sense), timeout_ms, mine, out, len(mine)))
        return [bytes(out[r * len(mine):(r + 1) * len(mine)]) for r in range(world)]

    def unlink(self):
        try:
            os.unlink(self.path)
        except OSError:
            pass


def dc_virtual_ranks(w):
    """flags value emulating w ranks of the multi-GPU divide-and-conquer path on one GPU"""
    return (w & 0xff) << 8


def set_nj_virtual_shards(w):
    """the next dist_matrix of a single-rank context emulates w unit-sharded ranks of the pruned NJ"""
    L = load_library()
    _chk(L, L.dpr_set_nj_virtual_shards(w))


def set_nj_mode(mode):
    """0 = full streaming scan every iteration, 1 = exact pruned scan (default)."""
    L = load_library()
    _chk(L, L.dpr_set_nj_mode(mode))


def set_nj_multi_plan(plan):
    """Several ranks, pruned NJ: 0 = auto (unit-sharded from 65 536 tips on), 1 = always unit-sharded, 2 = every rank
    runs the single-GPU plan."""
    L = load_library()
    _chk(L, L.dpr_set_nj_multi_plan(plan))


def _chk(L, rc):
    if rc < 0:
        raise DipperError(rc, (L.dpr_last_error() or b"").decode())
    return rc


(NJ_PLAN_SINGLE_STREAM, NJ_PLAN_SINGLE_PRUNED, NJ_PLAN_BIONJ, NJ_PLAN_ROWS_STREAM, NJ_PLAN_REPLICAS, NJ_PLAN_UNIT_SHARDED,
 NJ_PLAN_ROWS_PRUNED) = range(7)


def nj_plan_resolve(world, virtual_ranks, variant, pruned, multi_plan, virtual_shards, n, total_bytes):
    """the NJ plan (NJ_PLAN_*) that dist_matrix sets up for n tips under these knobs on a device of total_bytes (host only);
    raises DipperError where dist_matrix would refuse"""
    L = load_library()
    return _chk(L, L.dpr_nj_plan_resolve(world, int(virtual_ranks), variant, int(pruned), multi_plan, virtual_shards, n, total_bytes))


def place_policy_run(source, world, window_transport, no_overlap, multi_min, first, last, batch_rows, tree_ms, dist_alone_ms):
    """the overlap policy of place_run over a described run (host only): per batch of batch_rows tips from `first` on, whether its
    distance rows are produced beside the previous batch's tree kernels; tree_ms / dist_alone_ms: one figure per batch"""
    L = load_library()
    tree = np.ascontiguousarray(tree_ms, dtype=np.float64)
    dist = np.ascontiguousarray(dist_alone_ms, dtype=np.float64)
    assert tree.shape == dist.shape and tree.ndim == 1
    beside = np.zeros(max(len(tree), 1), dtype=np.int32)
    _chk(L, L.dpr_place_policy_run(source, world, int(window_transport), int(no_overlap), multi_min, first, last, batch_rows,
                                   _p(tree, c_f64p), _p(dist, c_f64p), len(tree), _p(beside, c_i32p)))
    return [bool(b) for b in beside[:len(tree)]]


def _p(a, t):
    return a.ctypes.data_as(t)


def pack4(seq: bytes):
    L = load_library()
    out = np.zeros((len(seq) + 15) // 16, dtype=np.uint64)
    _chk(L, L.dpr_pack4(seq, len(seq), _p(out, c_u64p)))
    return out


def pack2(seq: bytes):
    L = load_library()
    out = np.zeros((len(seq) + 31) // 32, dtype=np.uint64)
    _chk(L, L.dpr_pack2(seq, len(seq), _p(out, c_u64p)))
    return out


def pack_aa(seq: bytes):
    """one byte per site: ARNDCQEGHILKMFPSTWYV (either case) -> 0..19, everything else 255 (not a residue)"""
    L = load_library()
    out = np.zeros(len(seq), dtype=np.uint8)
    _chk(L, L.dpr_pack_aa(seq, len(seq), _p(out, C.POINTER(C.c_uint8))))
    return out


def pack_aa_many(seqs):
    """[n][L] codes, L = len(seqs[0]); a shorter sequence is padded with not-a-residue, a longer one cut"""
    Ls = len(seqs[0])
    out = np.full((len(seqs), Ls), 255, dtype=np.uint8)
    for i, s in enumerate(seqs):
        c = pack_aa(s)
        out[i, : min(Ls, len(c))] = c[:Ls]
    return out


def msa_boot_weights(seed, replicate, L):
    """multiplicity of every column of an L-site alignment in bootstrap replicate `replicate` (host only)"""
    lib = load_library()
    out = np.zeros(L, dtype=np.int32)
    _chk(lib, lib.dpr_msa_boot_weights(seed, replicate, L, _p(out, c_i32p)))
    return out


def split_support(n, main_x, main_y, rep_x, rep_y, counts=None):
    """counts[k] (internal node n+k of the main merge log) + 1 where the replicate's merge log has that node's split (host only)"""
    lib = load_library()
    k = max(n - 2, 1)
    mx, my, rx, ry = (np.ascontiguousarray(np.asarray(a, dtype=np.int32)[: n - 2]) for a in (main_x, main_y, rep_x, rep_y))
    if counts is None:
        counts = np.zeros(k, dtype=np.int32)
    assert counts.dtype == np.int32 and counts.flags.c_contiguous and len(counts) >= n - 2
    _chk(lib, lib.dpr_split_support(n, _p(mx, c_i32p), _p(my, c_i32p), _p(rx, c_i32p), _p(ry, c_i32p), _p(counts, c_i32p)))
    return counts


def _tbe_args(n, main_x, main_y, rep_x, rep_y, phi_sum):
    logs = [np.ascontiguousarray(np.asarray(a, dtype=np.int32)[: n - 2]) for a in (main_x, main_y, rep_x, rep_y)]
    if phi_sum is None:
        phi_sum = np.zeros(max(n - 2, 1), dtype=np.int64)
    assert phi_sum.dtype == np.int64 and phi_sum.flags.c_contiguous and len(phi_sum) >= n - 2
    return logs, phi_sum


def transfer_support_host(n, main_x, main_y, rep_x, rep_y, phi_sum=None):
    """phi_sum[k] (internal node n+k of the main merge log, min(|A|, n-|A|) >= 2) + the transfer distance phi of its clade to
    the replicate tree (host only)"""
    lib = load_library()
    (mx, my, rx, ry), phi_sum = _tbe_args(n, main_x, main_y, rep_x, rep_y, phi_sum)
    _chk(lib, lib.dpr_transfer_support_host(n, _p(mx, c_i32p), _p(my, c_i32p), _p(rx, c_i32p), _p(ry, c_i32p), _p(phi_sum, c_i64p)))
    return phi_sum


def _taxa_args(n, moved, pairs):
    if moved is None:
        moved = np.zeros(max(n, 1), dtype=np.int64)
    if pairs is None:
        pairs = np.zeros(1, dtype=np.int64)
    assert moved.dtype == np.int64 and moved.flags.c_contiguous and len(moved) >= n
    assert pairs.dtype == np.int64 and pairs.flags.c_contiguous and len(pairs) >= 1
    return moved, pairs


def transfer_taxa_host(n, main_x, main_y, rep_x, rep_y, cutoff_permille=300, phi_sum=None, moved=None, pairs=None):
    """(phi_sum, moved, pairs), each added to: phi as transfer_support_host; moved[t] + the counted branches (1000 phi <=
    cutoff_permille (p - 1)) whose transfer set holds tip t; pairs[0] + the counted branches (host only)"""
    lib = load_library()
    (mx, my, rx, ry), phi_sum = _tbe_args(n, main_x, main_y, rep_x, rep_y, phi_sum)
    moved, pairs = _taxa_args(n, moved, pairs)
    _chk(lib, lib.dpr_transfer_taxa_host(n, _p(mx, c_i32p), _p(my, c_i32p), _p(rx, c_i32p), _p(ry, c_i32p), cutoff_permille,
                                         _p(phi_sum, c_i64p), _p(moved, c_i64p), _p(pairs, c_i64p)))
    return phi_sum, moved, pairs


def _bme_args(n, merge_x, merge_y, max_rounds, nstats=4):
    mx, my = (np.ascontiguousarray(np.asarray(a, dtype=np.int32)[: max(n - 2, 0)]) for a in (merge_x, merge_y))
    assert len(mx) == len(my) == n - 2
    out = dict(kids=np.zeros(2 * max(n - 2, 1), dtype=np.int32), top=np.zeros(1, dtype=np.int32), len=np.zeros(2 * n - 2, dtype=np.float64),
               L_rounds=np.zeros(max_rounds + 1, dtype=np.float64), stats=np.zeros(nstats, dtype=np.int64))
    ptrs = (_p(mx, c_i32p), _p(my, c_i32p), max_rounds, _p(out["kids"], c_i32p), _p(out["top"], c_i32p), _p(out["len"], c_f64p),
            _p(out["L_rounds"], c_f64p), _p(out["stats"], c_i64p))
    return (mx, my), out, ptrs


def _bme_result(n, out):
    rounds, moves, fallbacks, cands0 = (int(v) for v in out["stats"][:4])
    more = dict(long_moves=int(out["stats"][4]), max_k=int(out["stats"][5])) if len(out["stats"]) == 6 else {}
    return dict(**more, kids=out["kids"][: 2 * (n - 2)].reshape(n - 2, 2), top=int(out["top"][0]), len=out["len"], L_rounds=out["L_rounds"][: rounds + 1],
                rounds=rounds, moves=moves, fallbacks=fallbacks, candidates0=cands0)


def bme_nni_host(D, merge_x, merge_y, max_rounds):
    """Balanced minimum evolution NNI search restated on the host (no GPU).  D: (n, n) array whose strict lower triangle is read;
    merge_x / merge_y: a merge log of n - 2 entries.  dict(kids (n-2, 2): children of node n+k hung from tip n-1; top: the node
    next to tip n-1; len (2n-2): balanced length of the edge above every node; L_rounds: the tree length before and after every
    accepted round; rounds, moves, fallbacks, candidates0)"""
    lib = load_library()
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    rows = np.ascontiguousarray(np.concatenate([D[i, :i] for i in range(n)])) if n > 1 else np.zeros(1)
    keep, out, ptrs = _bme_args(n, merge_x, merge_y, max_rounds)
    _chk(lib, lib.dpr_bme_nni_host(_p(rows, c_f64p), n, *ptrs))
    return _bme_result(n, out)


def bme_eval_host(D, kids, top):
    """one evaluation of the tree (kids, top) as bme_nni_host returns it (host only): dict(len, gain, move, L), 2n-2 entries each"""
    lib = load_library()
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    rows = np.ascontiguousarray(np.concatenate([D[i, :i] for i in range(n)]))
    kids = np.ascontiguousarray(np.asarray(kids, dtype=np.int32).reshape(-1))
    assert len(kids) == 2 * (n - 2)
    ln, gain, move = np.zeros(2 * n - 2), np.zeros(2 * n - 2), np.zeros(2 * n - 2, dtype=np.int32)
    L = C.c_double(0.0)
    _chk(lib, lib.dpr_bme_eval_host(_p(rows, c_f64p), n, _p(kids, c_i32p), int(top), _p(ln, c_f64p), _p(gain, c_f64p), _p(move, c_i32p), C.byref(L)))
    return dict(len=ln, gain=gain, move=move, L=L.value)


def _lower_rows(D):
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    return n, (np.ascontiguousarray(np.concatenate([D[i, :i] for i in range(n)])) if n > 1 else np.zeros(1))


def bme_spr_host(D, merge_x, merge_y, max_rounds):
    """Balanced minimum evolution SPR search restated on the host (no GPU): bme_nni_host's arguments and dict, with long_moves
    (applied moves that carried a subtree past k >= 2 edges) and max_k (the largest k applied) added"""
    lib = load_library()
    n, rows = _lower_rows(D)
    keep, out, ptrs = _bme_args(n, merge_x, merge_y, max_rounds, 6)
    _chk(lib, lib.dpr_bme_spr_host(_p(rows, c_f64p), n, *ptrs))
    return _bme_result(n, out)


def bme_spr_eval_host(D, kids, top):
    """one SPR scan of the tree (kids, top) (host only): dict(gain, w, k, L); per directed subtree d -- d = v: the clade of v,
    d = (2n-2) + v: outside the clade of v -- its best target's gain, lower node w and path length k (k = 0: none)"""
    lib = load_library()
    n, rows = _lower_rows(D)
    kids = np.ascontiguousarray(np.asarray(kids, dtype=np.int32).reshape(-1))
    assert len(kids) == 2 * (n - 2)
    m2 = 2 * (2 * n - 2)
    gain, w, k = np.zeros(m2), np.zeros(m2, dtype=np.int32), np.zeros(m2, dtype=np.int32)
    L = C.c_double(0.0)
    _chk(lib, lib.dpr_bme_spr_eval_host(_p(rows, c_f64p), n, _p(kids, c_i32p), int(top), _p(gain, c_f64p), _p(w, c_i32p), _p(k, c_i32p), C.byref(L)))
    return dict(gain=gain, w=w, k=k, L=L.value)


def bme_spr_gain_host(D, kids, top, d, w):
    """(gain, k) of the one SPR move that carries the directed subtree d onto the edge above w (host only); DipperError -1 if w
    is no target of d"""
    lib = load_library()
    n, rows = _lower_rows(D)
    kids = np.ascontiguousarray(np.asarray(kids, dtype=np.int32).reshape(-1))
    assert len(kids) == 2 * (n - 2)
    g, k = C.c_double(0.0), C.c_int32(0)
    _chk(lib, lib.dpr_bme_spr_gain_host(_p(rows, c_f64p), n, _p(kids, c_i32p), int(top), int(d), int(w), C.byref(g), C.byref(k)))
    return g.value, k.value


NJ_VARIANT_NJ, NJ_VARIANT_BIONJ = 0, 1


def upgma_host(D, linkage=0):
    """UPGMA (linkage 0) or WPGMA (1) restated naively on the host (no GPU).  D: (n, n) array whose strict lower triangle is read.
    dict(merge_x, merge_y, height), n - 1 entries each: the slots merged (the first n - 2 entries are an NJ-style merge log, the
    last one is the root) and the height of the node n + it they make"""
    lib = load_library()
    n, rows = _lower_rows(D)
    cnt = max(n - 1, 1)
    mx, my, h = np.zeros(cnt, dtype=np.int32), np.zeros(cnt, dtype=np.int32), np.zeros(cnt, dtype=np.float64)
    _chk(lib, lib.dpr_upgma_host(_p(rows, c_f64p), n, int(linkage), _p(mx, c_i32p), _p(my, c_i32p), _p(h, c_f64p)))
    return dict(merge_x=mx[: n - 1], merge_y=my[: n - 1], height=h[: n - 1])


PAIRS_STATS = ("blocks", "pairs", "components", "largest", "singletons", "peak_device_bytes")


def pairs_summary_host(label):
    """what the labels of pairs_within say (host only): dict(components, largest, singletons, rank) -- rank[v] the 1-based rank of v's
    cluster, clusters ordered by their smallest member"""
    lib = load_library()
    label = np.ascontiguousarray(label, dtype=np.int32)
    out, rank = np.zeros(3, dtype=np.int64), np.zeros(len(label), dtype=np.int32)
    _chk(lib, lib.dpr_pairs_summary_host(_p(label, c_i32p), len(label), _p(out, c_i64p), _p(rank, c_i32p)))
    return dict(components=int(out[0]), largest=int(out[1]), singletons=int(out[2]), rank=rank)


def pairs_within_host(D, threshold):
    """The pairs j < i of the strict lower triangle of the (n, n) array D with D[i, j] <= threshold, ordered by i then j, and
    label[v] = the smallest index of v's connected component, restated on the host (no GPU): dict(i, j, d, label, stats) as
    Dipper.pairs_within returns them (stats without blocks and peak_device_bytes)"""
    lib = load_library()
    n, rows = _lower_rows(D)
    count = C.c_int64(0)
    _chk(lib, lib.dpr_pairs_within_host(_p(rows, c_f64p), n, float(threshold), None, None, None, 0, C.byref(count), None))
    cap = max(count.value, 1)
    i, j, d, label = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap), np.zeros(n, dtype=np.int32)
    _chk(lib, lib.dpr_pairs_within_host(_p(rows, c_f64p), n, float(threshold), _p(i, c_i32p), _p(j, c_i32p), _p(d, c_f64p), cap, C.byref(count),
                                        _p(label, c_i32p)))
    k = count.value
    s = pairs_summary_host(label)
    return dict(i=i[:k], j=j[:k], d=d[:k], label=label,
                stats=dict(pairs=k, components=s["components"], largest=s["largest"], singletons=s["singletons"]))


NEAREST_STATS = ("blocks", "neighbours", "fewer", "none", "flushes", "peak_device_bytes")
NEAREST_MAX_K = 256


def nearest_host(D, K):
    """Each row's K nearest neighbours in the (n, n) array D, whose strict lower triangle is read as a symmetric matrix, restated on
    the host (no GPU): dict(j [n, K] int32, d [n, K], cnt [n] int32) as Dipper.nearest returns them.  Row i holds the columns c != i
    with a finite entry, by distance and then by column; behind the cnt[i] real places j is -1 and d the NaN 0x7ff8000000000000"""
    lib = load_library()
    n, rows = _lower_rows(D)
    K = int(K)
    size = max(n, 1) * min(max(K, 1), NEAREST_MAX_K)
    j, d, cnt = np.zeros(size, dtype=np.int32), np.zeros(size), np.zeros(max(n, 1), dtype=np.int32)
    _chk(lib, lib.dpr_nearest_host(_p(rows, c_f64p), n, K, _p(j, c_i32p), _p(d, c_f64p), _p(cnt, c_i32p)))
    return dict(j=j.reshape(n, K), d=d.reshape(n, K), cnt=cnt)


MST_STATS = ("rounds", "blocks", "edges", "components", "largest", "singletons", "peak_device_bytes", "rows_walked")


def mst_host(D):
    """The minimum spanning forest of the (n, n) array D, whose strict lower triangle is read as a symmetric matrix, by Kruskal on the
    host (no GPU): dict(i, j, d, label) as Dipper.mst returns them.  The E = n - components edges ascending by (key of the distance,
    i, j), i > j, d the entry's own bits; a NaN or infinite entry makes no edge; label[v] the smallest index of v's component"""
    lib = load_library()
    n, rows = _lower_rows(D)
    cap = max(n - 1, 1)
    i, j, d, label = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap), np.zeros(max(n, 1), dtype=np.int32)
    E = C.c_int64(0)
    _chk(lib, lib.dpr_mst_host(_p(rows, c_f64p), n, _p(i, c_i32p), _p(j, c_i32p), _p(d, c_f64p), C.byref(E), _p(label, c_i32p)))
    return dict(i=i[: E.value], j=j[: E.value], d=d[: E.value], label=label)


def mst_dendrogram_host(n, i, j, d):
    """The single-linkage dendrogram of a connected forest over n tips (the n - 1 edges of mst_host / Dipper.mst, in their order) as a
    merge log in the slot convention of upgma: dict(merge_x, merge_y, height), n - 1 entries each, height 0.5 * d.  tree_from_upgma
    takes it as it is.  Edges that do not connect the tips are refused"""
    lib = load_library()
    i, j = (np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1)) for a in (i, j))
    d = np.ascontiguousarray(np.asarray(d, dtype=np.float64).reshape(-1))
    assert len(i) == len(j) == len(d)
    cnt = max(int(n) - 1, 1)
    mx, my, h = np.zeros(cnt, dtype=np.int32), np.zeros(cnt, dtype=np.int32), np.zeros(cnt)
    _chk(lib, lib.dpr_mst_dendrogram_host(int(n), _p(i, c_i32p), _p(j, c_i32p), _p(d, c_f64p), len(i), _p(mx, c_i32p), _p(my, c_i32p), _p(h, c_f64p)))
    return dict(merge_x=mx[: n - 1], merge_y=my[: n - 1], height=h[: n - 1])


FIT_SUMS = ("n", "skipped", "sum_d", "sum_p", "sum_dd", "sum_pp", "sum_dp", "ss", "wss", "n_w", "max_e", "rms", "rms_rel", "explained",
            "cophenetic", "spare")


def _tree_args(n, parent, length):
    parent = np.ascontiguousarray(np.asarray(parent, dtype=np.int32).reshape(-1))
    length = np.ascontiguousarray(np.asarray(length, dtype=np.float64).reshape(-1))
    assert len(parent) == len(length)
    return parent, length, len(parent)


def _fit_result(out):
    sums, ss, pairs, worst = out
    return dict(sums=sums, taxon_ss=ss, taxon_pairs=pairs, worst=worst, **{k: float(sums[i]) for i, k in enumerate(FIT_SUMS)})


def _fit_out(n):
    out = (np.zeros(16), np.zeros(n), np.zeros(n, dtype=np.int64), np.zeros(2, dtype=np.int32))
    return out, (_p(out[0], c_f64p), _p(out[1], c_f64p), _p(out[2], c_i64p), _p(out[3], c_i32p))


def tree_fit_host(D, parent, length):
    """Fit of the tree (parent, length: m entries each, tips 0 .. n-1, parent -1 for the root) to the strict lower triangle of the
    (n, n) array D, restated on the host (no GPU).  dict(sums (16 doubles, also by the names of FIT_SUMS), taxon_ss, taxon_pairs,
    worst (i, j))"""
    lib = load_library()
    n, rows = _lower_rows(D)
    parent, length, m = _tree_args(n, parent, length)
    out, ptrs = _fit_out(n)
    _chk(lib, lib.dpr_tree_fit_host(_p(rows, c_f64p), n, m, _p(parent, c_i32p), _p(length, c_f64p), *ptrs))
    return _fit_result(out)


def tree_fit_derive(sums):
    """a copy of the 16 sums with the derived figures (entries 11 .. 15) computed from the first eleven"""
    lib = load_library()
    s = np.array(sums, dtype=np.float64)
    assert s.shape == (16,)
    _chk(lib, lib.dpr_tree_fit_derive(_p(s, c_f64p)))
    return s


def _tree_result(n, parent, length, m):
    return parent[: m.value], length[: m.value]


def tree_from_nj(merge_x, merge_y, bl_x, bl_y, last_d, n=None):
    """(parent, length) of an NJ / BIONJ merge log (n - 2 entries) with the node bookkeeping of the command's Newick writer: 2n - 1
    nodes, the two nodes left after the log under the root, each on 0.5 * last_d"""
    lib = load_library()
    mx, my = (np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1)) for a in (merge_x, merge_y))
    bx, by = (np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1)) for a in (bl_x, bl_y))
    n = len(mx) + 2 if n is None else int(n)
    assert n < 2 or len(mx) == len(my) == len(bx) == len(by) == n - 2
    if n == 2:
        mx = my = np.zeros(1, dtype=np.int32)
        bx = by = np.zeros(1)
    parent, length, m = np.zeros(max(2 * n - 1, 1), dtype=np.int32), np.zeros(max(2 * n - 1, 1)), C.c_int64(0)
    _chk(lib, lib.dpr_tree_from_nj(n, _p(mx, c_i32p), _p(my, c_i32p), _p(bx, c_f64p), _p(by, c_f64p), float(last_d), _p(parent, c_i32p),
                                   _p(length, c_f64p), C.byref(m)))
    return _tree_result(n, parent, length, m)


def tree_from_kids(kids, top, length):
    """(parent, length) of the outputs of bme_nni / bme_spr (kids: 2 (n - 2) entries, top, length: 2n - 2 entries): tip n - 1 and top
    under the root, each on half of length[top]"""
    lib = load_library()
    kids = np.ascontiguousarray(np.asarray(kids, dtype=np.int32).reshape(-1))
    ln = np.ascontiguousarray(np.asarray(length, dtype=np.float64).reshape(-1))
    n = len(ln) // 2 + 1
    assert len(ln) == 2 * n - 2 and len(kids) == 2 * max(n - 2, 0)
    if n == 2:
        kids = np.zeros(1, dtype=np.int32)
    parent, out, m = np.zeros(2 * n - 1, dtype=np.int32), np.zeros(2 * n - 1), C.c_int64(0)
    _chk(lib, lib.dpr_tree_from_kids(n, _p(kids, c_i32p), int(top), _p(ln, c_f64p), _p(parent, c_i32p), _p(out, c_f64p), C.byref(m)))
    return _tree_result(n, parent, out, m)


def tree_from_upgma(merge_x, merge_y, height):
    """(parent, length) of a UPGMA / WPGMA log (n - 1 entries): the rooted tree the command writes, the last merge the root"""
    lib = load_library()
    mx, my = (np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1)) for a in (merge_x, merge_y))
    h = np.ascontiguousarray(np.asarray(height, dtype=np.float64).reshape(-1))
    n = len(mx) + 1
    assert len(my) == len(h) == n - 1
    parent, length, m = np.zeros(max(2 * n - 1, 1), dtype=np.int32), np.zeros(max(2 * n - 1, 1)), C.c_int64(0)
    _chk(lib, lib.dpr_tree_from_upgma(n, _p(mx, c_i32p), _p(my, c_i32p), _p(h, c_f64p), _p(parent, c_i32p), _p(length, c_f64p), C.byref(m)))
    return _tree_result(n, parent, length, m)


def nj_variant_host(variant, D, max_iters=-1):
    """The streaming loop restated on the host (no GPU): variant 0 NJ, 1 BIONJ.  D: (n, n) array whose strict lower triangle is
    read.  dict(iters, merge_x, merge_y, bl_x, bl_y, last_d, lam): `iters` entries each; fewer than min(n - 2, max_iters) when an
    iteration found no candidate; lam is all 0.5 for NJ"""
    lib = load_library()
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    rows = np.ascontiguousarray(np.concatenate([D[i, :i] for i in range(n)])) if n > 1 else np.zeros(1)
    k = max(n - 2, 1)
    mx = np.zeros(k, dtype=np.int32)
    my = np.zeros(k, dtype=np.int32)
    bx = np.zeros(k, dtype=np.float64)
    by = np.zeros(k, dtype=np.float64)
    lam = np.full(k, 0.5, dtype=np.float64)
    last = C.c_double(0.0)
    done = _chk(lib, lib.dpr_nj_variant_host(variant, _p(rows, c_f64p), n, max_iters, _p(mx, c_i32p), _p(my, c_i32p), _p(bx, c_f64p),
                                             _p(by, c_f64p), C.byref(last), _p(lam, c_f64p)))
    return dict(iters=done, merge_x=mx[:done], merge_y=my[:done], bl_x=bx[:done], bl_y=by[:done], last_d=last.value, lam=lam[:done])


def pack4_many(seqs):
    """[n][ceil(L/16)] words, L = len(seqs[0]) (src/MSA.cu:19: every row uses sequence 0's length)."""
    Ls = len(seqs[0])
    W = (Ls + 15) // 16
    out = np.zeros((len(seqs), W), dtype=np.uint64)
    for i, s in enumerate(seqs):
        w = pack4(s)
        out[i, : min(W, len(w))] = w[:W]
    return out


class Dipper:
    """One GPU context (dpr_ctx)."""

    def __init__(self, device=0, virtual_world=0):
        self.L = load_library()
        h = C.c_void_p()
        if virtual_world:
            _chk(self.L, self.L.dpr_create_virtual(C.byref(h), device, virtual_world))
        else:
            _chk(self.L, self.L.dpr_create(C.byref(h), device))
        self.h = h

    def close(self):
        if self.h:
            self.L.dpr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def device_name(self):
        buf = C.create_string_buffer(256)
        _chk(self.L, self.L.dpr_device_name(self.h, buf, 256))
        return buf.value.decode()

    # ---- multi-GPU ------------------------------------------------------------------------------
    def comm_unique_id(self):
        buf = (C.c_char * 128)()
        _chk(self.L, self.L.dpr_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, rank, world, uid: bytes):
        buf = (C.c_char * 128).from_buffer_copy(uid) if uid else None
        _chk(self.L, self.L.dpr_comm_init(self.h, rank, world, buf))

    def comm_selftest(self):
        _chk(self.L, self.L.dpr_comm_selftest(self.h))

    def comm_init_local(self, rank, world):
        _chk(self.L, self.L.dpr_comm_init_local(self.h, rank, world))

    def comm_init_shared(self, rank, world, region, transport=0):
        """join `world` ranks through a shared host region (SharedRegion below); transport 0 auto, 1 RCCL, 2 ipc windows"""
        self._region = region          # (the mapping must outlive the context)
        _chk(self.L, self.L.dpr_comm_init_shared(self.h, rank, world, region.address, region.size, transport))

    def comm_stats(self):
        """(transport: 'none' | 'rccl' | 'ipc' | 'local', device collectives so far)"""
        t = C.c_int()
        n = C.c_int64()
        _chk(self.L, self.L.dpr_comm_stats(self.h, C.byref(t), C.byref(n)))
        return ["none", "rccl", "ipc", "local"][t.value], int(n.value)

    def peer_export(self, n_tips):
        buf = (C.c_char * 192)()
        _chk(self.L, self.L.dpr_peer_export(self.h, n_tips, buf))
        return bytes(buf)

    def peer_attach(self, blobs):
        data = b"".join(blobs)
        buf = (C.c_char * len(data)).from_buffer_copy(data)
        _chk(self.L, self.L.dpr_peer_attach(self.h, buf))

    def set_nj_exchange(self, plan):
        """row-sharded NJ loop: 0 legacy, 1 peer, 2 mailbox, -1 default"""
        _chk(self.L, self.L.dpr_ctx_set_nj_exchange(self.h, plan))

    def nj_exchange_info(self):
        p = C.c_int()
        nl = C.c_int64()
        nc = C.c_int64()
        note = C.create_string_buffer(256)
        _chk(self.L, self.L.dpr_get_nj_exchange_info(self.h, C.byref(p), C.byref(nl), C.byref(nc), note, 256))
        return {"plan": {0: "legacy", 1: "peer", 2: "mailbox"}.get(p.value, str(p.value)), "launches": int(nl.value),
                "collectives": int(nc.value), "note": note.value.decode()}

    def set_nj_adaptive(self, on):
        _chk(self.L, self.L.dpr_ctx_set_nj_adaptive(self.h, on))

    def nj_adaptive_stats(self):
        """(iterations run as streaming scans, epochs that switched) since the matrix was built"""
        a = C.c_int64()
        b = C.c_int64()
        _chk(self.L, self.L.dpr_get_nj_adaptive_stats(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def set_debug_fault(self, iteration, rank):
        """test hook of the one-exchange loops' cross-check: `rank` corrupts one pulled element at `iteration` (-1, -1: off)"""
        _chk(self.L, self.L.dpr_ctx_set_debug_fault(self.h, iteration, rank))

    def set_poll_limit_ms(self, ms):
        _chk(self.L, self.L.dpr_ctx_set_poll_limit_ms(self.h, ms))

    def comm_info(self):
        """(rank, ranks) as the RCCL communicator of this context reports them; (0, 1) without one"""
        r = C.c_int()
        n = C.c_int()
        _chk(self.L, self.L.dpr_comm_info(self.h, C.byref(r), C.byref(n)))
        return r.value, n.value

    # ---- inputs -----------------------------------------------------------------------------------
    def set_msa(self, packed4, L):
        p = np.ascontiguousarray(packed4, dtype=np.uint64)
        _chk(self.L, self.L.dpr_set_msa(self.h, _p(p, c_u64p), p.shape[0], L))
        self._msa_sites = int(L)      # (msa_site_coverage sizes its result by it)
        self._tips = {**getattr(self, "_tips", {}), SRC_MSA: int(p.shape[0])}      # (mst sizes its results by the source's tips)

    def set_msa_aa(self, codes):
        """protein alignment: codes [n][L] uint8 as pack_aa_many builds them (>= 20: not a residue); source stays SRC_MSA"""
        p = np.ascontiguousarray(codes, dtype=np.uint8)
        assert p.ndim == 2
        _chk(self.L, self.L.dpr_set_msa_aa(self.h, _p(p, C.POINTER(C.c_uint8)), p.shape[0], p.shape[1]))
        self._msa_sites = int(p.shape[1])
        self._tips = {**getattr(self, "_tips", {}), SRC_MSA: int(p.shape[0])}

    def set_matrix_lower(self, rows, n):
        r = np.ascontiguousarray(rows, dtype=np.float64)
        assert r.size == n * (n - 1) // 2
        _chk(self.L, self.L.dpr_set_matrix_lower(self.h, _p(r, c_f64p), n))
        self._tips = {**getattr(self, "_tips", {}), SRC_MATRIX: int(n)}

    def set_matrix_full(self, D):
        """Convenience: takes an (n,n) array and hands over its strict lower triangle row by row."""
        D = np.asarray(D, dtype=np.float64)
        n = D.shape[0]
        rows = np.concatenate([D[i, :i] for i in range(n)]) if n > 1 else np.zeros(0)
        self.set_matrix_lower(rows, n)

    def set_reads(self, seqs):
        """seqs: list of byte strings (unaligned reads); packs with the 2-bit encoder."""
        words = [pack2(s) for s in seqs]
        lens = np.array([len(s) for s in seqs], dtype=np.uint64)
        nw = np.array([len(w) for w in words], dtype=np.uint64)
        off = np.zeros(len(seqs), dtype=np.uint64)
        off[1:] = np.cumsum(nw)[:-1]
        flat = np.concatenate(words) if len(words) else np.zeros(0, np.uint64)
        if flat.size == 0:
            flat = np.zeros(1, np.uint64)
        self._reads = (np.ascontiguousarray(flat), off, lens)
        _chk(self.L, self.L.dpr_set_reads(self.h, _p(self._reads[0], c_u64p), _p(off, c_u64p), _p(lens, c_u64p), len(seqs)))
        self._tips = {**getattr(self, "_tips", {}), SRC_MASH: len(seqs)}

    def set_reads_packed(self, flat, off, lens):
        """already 2-bit packed reads: the three arrays of dpr_set_reads (twoBitCompressor layout)"""
        flat = np.ascontiguousarray(flat, dtype=np.uint64)
        off = np.ascontiguousarray(off, dtype=np.uint64)
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        self._reads = (flat, off, lens)
        _chk(self.L, self.L.dpr_set_reads(self.h, _p(flat, c_u64p), _p(off, c_u64p), _p(lens, c_u64p), len(lens)))
        self._tips = {**getattr(self, "_tips", {}), SRC_MASH: len(lens)}

    def sketch(self, k=15, S=1000, fetch=True):
        n = len(self._reads[2])
        out = np.zeros((n, S), dtype=np.uint64) if fetch else None
        _chk(self.L, self.L.dpr_sketch(self.h, k, S, _p(out, c_u64p) if fetch else None))
        return out

    def mash_index_info(self):
        """the inverted index of the last sketch call and its kernel's constants (dpr_get_mash_index_info)"""
        info = np.zeros(8, dtype=np.int64)
        _chk(self.L, self.L.dpr_get_mash_index_info(self.h, _p(info, c_i64p)))
        names = ("built", "chunk_tips", "chunks", "distinct", "dense", "dense_min", "max_sketch", "beside_task_bound")
        return {nm: int(v) for nm, v in zip(names, info)}

    def kmer_hashes(self, seq, k):
        _, off, lens = self._reads
        nk = max(int(lens[seq]) - k + 1, 0)
        out = np.zeros(max(nk, 1), dtype=np.uint64)
        _chk(self.L, self.L.dpr_get_kmer_hashes(self.h, seq, k, _p(off, c_u64p), _p(lens, c_u64p), _p(out, c_u64p)))
        return out[:nk]

    def place_run(self, source, n, first=2, dist_type=1, k=15, state=None):
        st = state or dict(head=np.full(2 * n, -1, np.int32), e=np.full(8 * n, -1, np.int32),
                           nxt=np.full(8 * n, -1, np.int32), belong=np.full(8 * n, -1, np.int32),
                           len=np.full(8 * n, 2.0, np.float64))
        _chk(self.L, self.L.dpr_place_run(self.h, source, dist_type, k, first, n, _p(st["head"], c_i32p),
                                          _p(st["e"], c_i32p), _p(st["nxt"], c_i32p), _p(st["belong"], c_i32p),
                                          _p(st["len"], c_f64p)))
        cid = np.zeros(40 * n, np.int32)
        cdis = np.zeros(40 * n, np.float64)
        trace = np.zeros(3 * n, np.float64)
        _chk(self.L, self.L.dpr_get_place_state(self.h, _p(cid, c_i32p), _p(cdis, c_f64p), _p(trace, c_f64p)))
        st.update(cid=cid, cdis=cdis, trace=trace.reshape(n, 3))
        return st

    def place_exact_run(self, source, n, dist_type=1, k=15):
        """Exact placement mode (dpr_place_exact_run); returns adjacency, rev, dep, trace."""
        st = dict(head=np.full(2 * n, -1, np.int32), e=np.full(8 * n, -1, np.int32),
                  nxt=np.full(8 * n, -1, np.int32), belong=np.full(8 * n, -1, np.int32),
                  len=np.full(8 * n, 2.0, np.float64))
        _chk(self.L, self.L.dpr_place_exact_run(self.h, source, dist_type, k, n, _p(st["head"], c_i32p),
                                                _p(st["e"], c_i32p), _p(st["nxt"], c_i32p),
                                                _p(st["belong"], c_i32p), _p(st["len"], c_f64p)))
        rev = np.zeros(8 * n, np.int32)
        dep = np.zeros(2 * n, np.int32)
        trace = np.zeros(3 * n, np.float64)
        _chk(self.L, self.L.dpr_get_exact_state(self.h, _p(rev, c_i32p), _p(dep, c_i32p)))
        _chk(self.L, self.L.dpr_get_place_state(self.h, None, None, _p(trace, c_f64p)))
        st.update(rev=rev, dep=dep, trace=trace.reshape(n, 3))
        return st

    def dc_run(self, source, n, backbone, dist_type=1, k=15, flags=0):
        """Divide-and-conquer mode (dpr_dc_run); returns the adjacency, closest lists, trace, cluster ids."""
        st = dict(head=np.full(2 * n, -1, np.int32), e=np.full(8 * n, -1, np.int32),
                  nxt=np.full(8 * n, -1, np.int32), belong=np.full(8 * n, -1, np.int32),
                  len=np.full(8 * n, 2.0, np.float64))
        cl = np.full(n, -1, np.int32)
        _chk(self.L, self.L.dpr_dc_run(self.h, source, dist_type, k, n, backbone, flags, _p(st["head"], c_i32p),
                                       _p(st["e"], c_i32p), _p(st["nxt"], c_i32p), _p(st["belong"], c_i32p),
                                       _p(st["len"], c_f64p), _p(cl, c_i32p)))
        cid = np.zeros(40 * n, np.int32)
        cdis = np.zeros(40 * n, np.float64)
        trace = np.zeros(3 * n, np.float64)
        _chk(self.L, self.L.dpr_get_place_state(self.h, _p(cid, c_i32p), _p(cdis, c_f64p), _p(trace, c_f64p)))
        counts = np.zeros(5, np.int64)
        ms = np.zeros(3, np.float64)
        _chk(self.L, self.L.dpr_get_dc_stats(self.h, counts.ctypes.data_as(C.POINTER(C.c_int64)), _p(ms, c_f64p)))
        st.update(cid=cid, cdis=cdis, trace=trace.reshape(n, 3), cluster_id=cl,
                  stats=dict(clusters=int(counts[0]), max_cluster=int(counts[1]), pairs=int(counts[2]),
                             groups=int(counts[3]), jobs=int(counts[4]), backbone_ms=float(ms[0]),
                             assign_ms=float(ms[1]), cluster_ms=float(ms[2])))
        return st

    def dc_table_stats(self):
        """the assignment table of the last dc_run (dpr_get_dc_table_stats)"""
        out = np.zeros(4, dtype=np.int64)
        _chk(self.L, self.L.dpr_get_dc_table_stats(self.h, _p(out, c_i64p)))
        return {nm: int(v) for nm, v in zip(("entries", "chunks", "max_entries", "max_leaves"), out)}

    def place_fixed_set(self, m, n, state):
        """dpr_place_fixed_set: the backbone of m tips (adjacency arrays of `state`, sized for n tips) becomes the context's
        fixed backbone"""
        st = {k: np.ascontiguousarray(state[k], dtype=np.float64 if k == "len" else np.int32) for k in ("head", "e", "nxt", "belong", "len")}
        assert st["head"].size >= 2 * n and all(st[k].size >= 8 * n for k in ("e", "nxt", "belong", "len"))
        _chk(self.L, self.L.dpr_place_fixed_set(self.h, m, n, _p(st["head"], c_i32p), _p(st["e"], c_i32p), _p(st["nxt"], c_i32p),
                                                _p(st["belong"], c_i32p), _p(st["len"], c_f64p)))
        self._pfix_nq = n - m

    def place_fixed_run(self, source, dist_type=1, k=15):
        """dpr_place_fixed_run: (slot, frac, add) of every query against the context's current input"""
        nq = max(getattr(self, "_pfix_nq", 1), 1)      # (never set: one entry, the library reports the state error)
        slot = np.full(nq, -2, np.int32)
        frac = np.zeros(nq, np.float64)
        add = np.zeros(nq, np.float64)
        _chk(self.L, self.L.dpr_place_fixed_run(self.h, source, dist_type, k, _p(slot, c_i32p), _p(frac, c_f64p), _p(add, c_f64p)))
        return slot, frac, add

    def set_place_fixed_batch(self, queries):
        _chk(self.L, self.L.dpr_ctx_set_place_fixed_batch(self.h, queries))

    def place_fixed_timing(self):
        """(distance blocks, scan + reduce) of the last place_fixed_run in milliseconds"""
        a = C.c_double()
        b = C.c_double()
        _chk(self.L, self.L.dpr_get_place_fixed_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def warm_graphs(self):
        _chk(self.L, self.L.dpr_warm_graphs(self.h))

    def reserve_nj(self, n):
        _chk(self.L, self.L.dpr_reserve_nj(self.h, n))

    def dist_matrix(self, source, dist_type=1, k=15):
        _chk(self.L, self.L.dpr_dist_matrix(self.h, source, dist_type, k))

    # ---- NJ ---------------------------------------------------------------------------------------
    def nj_run(self, max_iters=-1):
        N = self.L.dpr_n_total(self.h)
        k = max(N - 2, 1)
        mx = np.zeros(k, dtype=np.int32)
        my = np.zeros(k, dtype=np.int32)
        bx = np.zeros(k, dtype=np.float64)
        by = np.zeros(k, dtype=np.float64)
        last = C.c_double(0.0)
        done = _chk(self.L, self.L.dpr_nj_run(self.h, max_iters, _p(mx, c_i32p), _p(my, c_i32p),
                                              _p(bx, c_f64p), _p(by, c_f64p), C.byref(last)))
        return dict(iters=done, merge_x=mx[:done], merge_y=my[:done], bl_x=bx[:done], bl_y=by[:done],
                    last_d=last.value)

    def nj_run_partial(self, max_iters=-1):
        """like nj_run, but a run that ends without a Q candidate (DPR_ERR_NOCAND: the reference's undefined (0,0) merge) returns
        the log up to there instead of raising: dict(..., code=0 or -4)"""
        N = self.L.dpr_n_total(self.h)
        k = max(N - 2, 1)
        mx = np.zeros(k, dtype=np.int32)
        my = np.zeros(k, dtype=np.int32)
        bx = np.zeros(k, dtype=np.float64)
        by = np.zeros(k, dtype=np.float64)
        last = C.c_double(0.0)
        it0, _ = self.nj_progress()
        rc = self.L.dpr_nj_run(self.h, max_iters, _p(mx, c_i32p), _p(my, c_i32p), _p(bx, c_f64p), _p(by, c_f64p), C.byref(last))
        if rc < 0 and rc != -4:
            _chk(self.L, rc)
        done = self.nj_progress()[0] - it0
        return dict(iters=done, code=0 if rc >= 0 else int(rc), merge_x=mx[:done], merge_y=my[:done], bl_x=bx[:done], bl_y=by[:done],
                    last_d=last.value)

    def nj_progress(self):
        """(iterations done since dist_matrix, active size)"""
        a = C.c_int64()
        b = C.c_int64()
        _chk(self.L, self.L.dpr_get_nj_progress(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def njp_shape(self):
        """launch shape of the pruned path's current epoch: dict(positions, row_groups, strips, post2, scan_grid)"""
        P = C.c_int64()
        v = [C.c_int() for _ in range(4)]
        _chk(self.L, self.L.dpr_get_njp_shape(self.h, C.byref(P), *[C.byref(x) for x in v]))
        return dict(positions=int(P.value), row_groups=v[0].value, strips=v[1].value, post2=bool(v[2].value), scan_grid=v[3].value)

    def nj_multi_info(self):
        buf = C.create_string_buffer(256)
        _chk(self.L, self.L.dpr_get_nj_multi_info(self.h, buf, 256))
        return buf.value.decode()

    def nj_is_unit_sharded(self):
        return bool(self.L.dpr_nj_is_unit_sharded(self.h))

    # plan knobs of THIS context (-1 = follow the process-wide default); effective at the next dist_matrix
    def set_nj_mode(self, mode):
        _chk(self.L, self.L.dpr_ctx_set_nj_mode(self.h, mode))

    def set_nj_multi_plan(self, plan):
        _chk(self.L, self.L.dpr_ctx_set_nj_multi_plan(self.h, plan))

    def set_nj_virtual_shards(self, w):
        _chk(self.L, self.L.dpr_ctx_set_nj_virtual_shards(self.h, w))

    def set_nj_variant(self, variant):
        """0 = NJ (default), 1 = BIONJ; effective at the next dist_matrix / reserve_nj"""
        _chk(self.L, self.L.dpr_ctx_set_nj_variant(self.h, variant))

    def nj_lambda(self):
        """lambda of the BIONJ iterations done since dist_matrix"""
        out = np.zeros(max(self.n_total() - 2, 1), dtype=np.float64)
        cnt = C.c_int64()
        _chk(self.L, self.L.dpr_get_nj_lambda(self.h, _p(out, c_f64p), C.byref(cnt)))
        return out[: cnt.value]

    def argmin_once(self, reps=1):
        i = C.c_int32()
        j = C.c_int32()
        q = C.c_double()
        ms = C.c_float()
        _chk(self.L, self.L.dpr_argmin_once(self.h, reps, C.byref(i), C.byref(j), C.byref(q), C.byref(ms)))
        return i.value, j.value, q.value, ms.value

    def set_nj_kernel_timing(self, stride):
        _chk(self.L, self.L.dpr_ctx_set_nj_kernel_timing(self.h, stride))

    def nj_kernel_timing(self):
        """per-kernel averages of the last timed NJ run (set_nj_kernel_timing): launch order, microseconds"""
        nk = C.c_int()
        ns = C.c_int64()
        us = np.zeros(8, np.float64)
        _chk(self.L, self.L.dpr_get_nj_kernel_timing(self.h, C.byref(nk), _p(us, c_f64p), C.byref(ns)))
        names = [(self.L.dpr_nj_kernel_name(i) or b"").decode() for i in range(nk.value)]
        rec = {"kernels_per_iteration": sum(1 for nm in names if not nm.startswith("(")), "sampled_iterations": int(ns.value),
               "kernel_us_avg": {nm: float(us[i]) for i, nm in enumerate(names)}}
        for i, nm in enumerate(names):
            if "scan" in nm:
                rec["scan_kernel"], rec["scan_us_avg"] = nm, float(us[i])
        return rec

    def place_walks(self):
        """(reached[n], dict(spilled, largest, total, degree_walks)) of the last placement run's closest-list walks"""
        st = (C.c_int64 * 6)()
        _chk(self.L, self.L.dpr_get_place_walks(self.h, None, st))
        return dict(spilled=int(st[0]), largest=int(st[1]), total=int(st[2]), degree_walks=int(st[3]), full_eval_dirty=int(st[4]), full_eval_rescans=int(st[5]))

    def place_walks_per_tip(self, n):
        out = np.zeros(n, dtype=np.int32)
        st = (C.c_int64 * 6)()
        _chk(self.L, self.L.dpr_get_place_walks(self.h, _p(out, c_i32p), st))
        return out

    def place_timing(self):
        a = C.c_double()
        b = C.c_double()
        _chk(self.L, self.L.dpr_get_place_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def place_overlap(self):
        """(overlapped, dist_busy_ms): whether the last placement run computed its distance rows beside the tree kernels,
        and for how long those batches were in flight (not a summand of the wall time)"""
        o = C.c_int()
        b = C.c_double()
        _chk(self.L, self.L.dpr_get_place_overlap(self.h, C.byref(o), C.byref(b)))
        return bool(o.value), b.value

    def place_policy(self):
        """(batches, batches produced beside the previous batch's tree kernels) of the last placement run"""
        a = C.c_int64()
        b = C.c_int64()
        _chk(self.L, self.L.dpr_get_place_policy(self.h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # ---- hooks ------------------------------------------------------------------------------------
    def n_active(self):
        return _chk(self.L, self.L.dpr_n_active(self.h))

    def n_total(self):
        return self.L.dpr_n_total(self.h)

    def matrix_row(self, i):
        out = np.zeros(self.n_total(), dtype=np.float64)
        _chk(self.L, self.L.dpr_get_matrix_row(self.h, i, _p(out, c_f64p)))
        return out

    def matrix(self):
        n = self.n_total()
        out = np.zeros((n, n), dtype=np.float64)
        for i in range(n):
            _chk(self.L, self.L.dpr_get_matrix_row(self.h, i, _p(out[i], c_f64p)))
        return out

    def row_sums(self):
        out = np.zeros(self.n_total(), dtype=np.float64)
        _chk(self.L, self.L.dpr_get_row_sums(self.h, _p(out, c_f64p)))
        return out

    def msa_dist_block(self, row0, nrows, ncols, dist_type=2, transposed=False, fetch=True, reps=1):
        """(block or None, average milliseconds per launch)"""
        out = np.zeros((ncols, nrows) if transposed else (nrows, ncols), dtype=np.float64) if fetch else None
        ms = C.c_float()
        _chk(self.L, self.L.dpr_msa_dist_block(self.h, row0, nrows, ncols, dist_type, 1 if transposed else 0,
                                               _p(out, c_f64p) if fetch else None, reps, C.byref(ms)))
        return out, ms.value

    def msa_resample(self, seed, replicate):
        """the MSA planes become those of bootstrap replicate `replicate` (-1: the uploaded alignment again)"""
        _chk(self.L, self.L.dpr_msa_resample(self.h, seed, replicate))

    def msa_boot_weights(self, L):
        """the active replicate's column multiplicities as the device computed them"""
        out = np.zeros(L, dtype=np.int32)
        _chk(self.L, self.L.dpr_get_msa_boot_weights(self.h, _p(out, c_i32p)))
        return out

    def msa_site_coverage(self):
        """cov[c]: the sequences of the current alignment that hold a symbol at column c (one entry per site)"""
        sites = getattr(self, "_msa_sites", 0)
        if not sites:
            raise DipperError(-3, "msa_site_coverage: call set_msa or set_msa_aa first")
        out = np.zeros(sites, dtype=np.int32)
        _chk(self.L, self.L.dpr_get_msa_site_coverage(self.h, _p(out, c_i32p)))
        return out

    def msa_filter_sites(self, permille):
        """keeps the columns with 1000 cov >= permille n (1000: complete deletion), on the device; returns the sites kept"""
        self._msa_sites = int(_chk(self.L, self.L.dpr_msa_filter_sites(self.h, permille)))
        return self._msa_sites

    def comm_sum_i32(self, values):
        """in-place integer sum over the context's ranks"""
        a = np.ascontiguousarray(values, dtype=np.int32)
        _chk(self.L, self.L.dpr_comm_sum_i32(self.h, _p(a, c_i32p), len(a)))
        return a

    def transfer_support(self, n, main_x, main_y, rep_x, rep_y, phi_sum=None):
        """transfer_support_host's numbers, computed on the device"""
        (mx, my, rx, ry), phi_sum = _tbe_args(n, main_x, main_y, rep_x, rep_y, phi_sum)
        _chk(self.L, self.L.dpr_transfer_support(self.h, n, _p(mx, c_i32p), _p(my, c_i32p), _p(rx, c_i32p), _p(ry, c_i32p),
                                                 _p(phi_sum, c_i64p)))
        return phi_sum

    def bme_nni(self, merge_x, merge_y, max_rounds):
        """bme_nni_host's result, computed on the device from the context's fresh matrix (after dist_matrix, before nj_run)"""
        n = len(np.asarray(merge_x)) + 2
        keep, out, ptrs = _bme_args(n, merge_x, merge_y, max_rounds)
        _chk(self.L, self.L.dpr_bme_nni(self.h, n, *ptrs))
        return _bme_result(n, out)

    def bme_spr(self, merge_x, merge_y, max_rounds):
        """bme_spr_host's result, computed on the device from the context's fresh matrix (after dist_matrix, before nj_run)"""
        n = len(np.asarray(merge_x)) + 2
        keep, out, ptrs = _bme_args(n, merge_x, merge_y, max_rounds, 6)
        _chk(self.L, self.L.dpr_bme_spr(self.h, n, *ptrs))
        return _bme_result(n, out)

    def bme_spr_timing(self):
        """scan ms of the last bme_spr, summed over its evaluations (bme_timing gives the table and lengths of the same call)"""
        a = C.c_double()
        _chk(self.L, self.L.dpr_get_bme_spr_timing(self.h, C.byref(a)))
        return a.value

    def bme_spr_stats(self):
        """dict(stack_bytes, allocations so far beyond the table's, scan launches of the last bme_spr, workers)"""
        out = np.zeros(4, dtype=np.int64)
        _chk(self.L, self.L.dpr_get_bme_spr_stats(self.h, _p(out, c_i64p)))
        return dict(stack_bytes=int(out[0]), allocations=int(out[1]), launches=int(out[2]), workers=int(out[3]))

    def bme_timing(self):
        """(table ms, lengths + gains ms) of the last bme_nni, summed over its evaluations"""
        a = C.c_double()
        b = C.c_double()
        _chk(self.L, self.L.dpr_get_bme_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def bme_stats(self):
        """dict(table_bytes, allocations so far, launches and evaluations of the last bme_nni)"""
        out = np.zeros(4, dtype=np.int64)
        _chk(self.L, self.L.dpr_get_bme_stats(self.h, _p(out, c_i64p)))
        return dict(table_bytes=int(out[0]), allocations=int(out[1]), launches=int(out[2]), evaluations=int(out[3]))

    def upgma(self, linkage=0):
        """upgma_host's result, computed on the device from the context's fresh matrix (after dist_matrix, before nj_run); the
        context's matrix is left as it was"""
        n = self.n_total()
        cnt = max(n - 1, 1)
        mx, my, h = np.zeros(cnt, dtype=np.int32), np.zeros(cnt, dtype=np.int32), np.zeros(cnt, dtype=np.float64)
        done = self.L.dpr_upgma_run(self.h, int(linkage), _p(mx, c_i32p), _p(my, c_i32p), _p(h, c_f64p))
        if done < 0:
            _chk(self.L, int(done))
        return dict(merge_x=mx[:done], merge_y=my[:done], height=h[:done])

    def upgma_stats(self):
        """dict(bytes held, allocations so far, launches and rows rescanned of the last upgma)"""
        out = np.zeros(4, dtype=np.int64)
        _chk(self.L, self.L.dpr_get_upgma_stats(self.h, _p(out, c_i64p)))
        return dict(bytes=int(out[0]), allocations=int(out[1]), launches=int(out[2]), rescanned=int(out[3]))

    def upgma_timing(self):
        """ms of the n - 1 iterations of the last upgma (HIP events)"""
        a = C.c_double()
        _chk(self.L, self.L.dpr_get_upgma_timing(self.h, C.byref(a)))
        return a.value

    def pairs_begin(self, source, dist_type=1, k=15, threshold=0.0, block_rows=0):
        _chk(self.L, self.L.dpr_pairs_begin(self.h, source, dist_type, k, float(threshold), int(block_rows)))

    def pairs_next(self, copy=True):
        """(i, j, d, rows_done) of the next row block: copies of the library's pinned arrays (copy=False: views, valid until the next call)"""
        pi, pj, pd = c_i32p(), c_i32p(), c_f64p()
        cnt, done = C.c_int64(0), C.c_int64(0)
        _chk(self.L, self.L.dpr_pairs_next(self.h, C.byref(pi), C.byref(pj), C.byref(pd), C.byref(cnt), C.byref(done)))
        k = cnt.value
        if k == 0:
            return np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0), done.value
        out = [np.ctypeslib.as_array(p, (k,)) for p in (pi, pj, pd)]
        return (*[a.copy() if copy else a for a in out], done.value)

    def pairs_labels(self, n):
        label = np.zeros(n, dtype=np.int32)
        _chk(self.L, self.L.dpr_pairs_labels(self.h, _p(label, c_i32p)))
        return label

    def pairs_stats(self):
        out = np.zeros(6, dtype=np.int64)
        _chk(self.L, self.L.dpr_pairs_stats(self.h, _p(out, c_i64p)))
        return {k: int(out[t]) for t, k in enumerate(PAIRS_STATS)}

    def pairs_info(self):
        """dict(dist_ms, filter_ms, copy_ms, block_rows, n) of the stream so far (ms: HIP events, summed over its blocks)"""
        ms, shape = np.zeros(3), np.zeros(2, dtype=np.int64)
        _chk(self.L, self.L.dpr_get_pairs_info(self.h, _p(ms, c_f64p), _p(shape, c_i64p)))
        return dict(dist_ms=float(ms[0]), filter_ms=float(ms[1]), copy_ms=float(ms[2]), block_rows=int(shape[0]), n=int(shape[1]))

    def pairs_end(self):
        _chk(self.L, self.L.dpr_pairs_end(self.h))

    def pairs_within(self, source, dist_type=1, k=15, threshold=0.0, block_rows=0, keep=True):
        """The pairs j < i within `threshold` of the uploaded source (alignment, sketches, or the matrix of set_matrix_lower), ordered
        by i then j, streamed in blocks of block_rows rows (0: the library's choice) without ever building the matrix, and the
        single-linkage clusters they form: dict(i, j, d, label, stats, info).  label[v] is the smallest index of v's cluster; stats
        has the keys of PAIRS_STATS, info those of pairs_info.  keep=False: the pairs are counted and dropped (measurement runs)"""
        self.pairs_begin(source, dist_type, k, threshold, block_rows)
        try:
            n = self.pairs_info()["n"]
            parts, done = [], 0
            while done < n:
                pi, pj, pd, done = self.pairs_next(copy=keep)
                if len(pi) and keep:
                    parts.append((pi, pj, pd))
            label = self.pairs_labels(n)
            stats, info = self.pairs_stats(), self.pairs_info()
        finally:
            self.pairs_end()
        cat = (lambda t, dt: np.concatenate([p[t] for p in parts]) if parts else np.zeros(0, dtype=dt))
        return dict(i=cat(0, np.int32), j=cat(1, np.int32), d=cat(2, np.float64), label=label, stats=stats, info=info)

    def nearest_begin(self, source, dist_type=1, k=15, K=10, block_rows=0):
        _chk(self.L, self.L.dpr_nearest_begin(self.h, source, dist_type, k, int(K), int(block_rows)))

    def nearest_next(self, K, copy=True):
        """(j [rows, K], d [rows, K], cnt [rows], row0) of the next row block: copies of the library's pinned arrays (copy=False:
        views, valid until the next call); rows == 0 behind the last block"""
        pj, pd, pc = c_i32p(), c_f64p(), c_i32p()
        row0, rows = C.c_int64(0), C.c_int64(0)
        _chk(self.L, self.L.dpr_nearest_next(self.h, C.byref(pj), C.byref(pd), C.byref(pc), C.byref(row0), C.byref(rows)))
        r = rows.value
        if r == 0:
            return np.zeros((0, K), dtype=np.int32), np.zeros((0, K)), np.zeros(0, dtype=np.int32), row0.value
        out = [np.ctypeslib.as_array(pj, (r, K)), np.ctypeslib.as_array(pd, (r, K)), np.ctypeslib.as_array(pc, (r,))]
        return (*[a.copy() if copy else a for a in out], row0.value)

    def nearest_stats(self):
        out = np.zeros(6, dtype=np.int64)
        _chk(self.L, self.L.dpr_nearest_stats(self.h, _p(out, c_i64p)))
        return {k: int(out[t]) for t, k in enumerate(NEAREST_STATS)}

    def nearest_info(self):
        """dict(dist_ms, select_ms, copy_ms, block_rows, n) of the stream so far (ms: HIP events, summed over its blocks)"""
        ms, shape = np.zeros(3), np.zeros(2, dtype=np.int64)
        _chk(self.L, self.L.dpr_get_nearest_info(self.h, _p(ms, c_f64p), _p(shape, c_i64p)))
        return dict(dist_ms=float(ms[0]), select_ms=float(ms[1]), copy_ms=float(ms[2]), block_rows=int(shape[0]), n=int(shape[1]))

    def nearest_end(self):
        _chk(self.L, self.L.dpr_nearest_end(self.h))

    def nearest(self, source, dist_type=1, k=15, K=10, block_rows=0, keep=True):
        """The K nearest neighbours of every sequence of the uploaded source (alignment, sketches, or the matrix of set_matrix_lower),
        streamed in blocks of block_rows full rows (0: the library's choice) without ever building the matrix: dict(j [n, K], d [n, K],
        cnt [n], stats, info).  Row i: the columns c != i with a finite distance, nearest first, equal distances by column; behind the
        cnt[i] real places j is -1 and d NaN.  stats has the keys of NEAREST_STATS, info those of nearest_info.  keep=False: the blocks
        are dropped (measurement runs)"""
        self.nearest_begin(source, dist_type, k, K, block_rows)
        try:
            n = self.nearest_info()["n"]
            parts, done = [], 0
            while done < n:
                pj, pd, pc, row0 = self.nearest_next(K, copy=keep)
                assert row0 == done and len(pc) > 0
                done += len(pc)
                if keep:
                    parts.append((pj, pd, pc))
            stats, info = self.nearest_stats(), self.nearest_info()
        finally:
            self.nearest_end()
        if not keep:
            return dict(j=None, d=None, cnt=None, stats=stats, info=info)
        return dict(j=np.concatenate([p[0] for p in parts]), d=np.concatenate([p[1] for p in parts]),
                    cnt=np.concatenate([p[2] for p in parts]), stats=stats, info=info)

    def mst_stats(self):
        out = np.zeros(8, dtype=np.int64)
        _chk(self.L, self.L.dpr_mst_stats(self.h, _p(out, c_i64p)))
        return {k: int(out[t]) for t, k in enumerate(MST_STATS)}

    def mst_info(self):
        """dict(dist_ms, rowmin_ms, round_ms, block_rows, n) of the last mst (ms: HIP events, summed over its rounds)"""
        ms, shape = np.zeros(3), np.zeros(2, dtype=np.int64)
        _chk(self.L, self.L.dpr_get_mst_info(self.h, _p(ms, c_f64p), _p(shape, c_i64p)))
        return dict(dist_ms=float(ms[0]), rowmin_ms=float(ms[1]), round_ms=float(ms[2]), block_rows=int(shape[0]), n=int(shape[1]))

    def mst(self, source, dist_type=1, k=15, block_rows=0):
        """The minimum spanning forest of the distances of the uploaded source (alignment, sketches, or the matrix of set_matrix_lower),
        by Boruvka rounds over streamed blocks of block_rows full rows (0: the library's choice) without ever building the matrix:
        dict(i, j, d, label, stats, info).  The edges ascending by (key of the distance, i, j), i > j; label[v] the smallest index of
        v's component; stats has the keys of MST_STATS, info those of mst_info"""
        n = getattr(self, "_tips", {}).get(source, 0)      # (nothing uploaded: the library says so)
        cap = max(n - 1, 1)
        i, j, d, label = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32), np.zeros(cap), np.zeros(max(n, 1), dtype=np.int32)
        E = C.c_int64(0)
        _chk(self.L, self.L.dpr_mst_run(self.h, source, dist_type, k, int(block_rows), _p(i, c_i32p), _p(j, c_i32p), _p(d, c_f64p), C.byref(E),
                                        _p(label, c_i32p)))
        return dict(i=i[: E.value], j=j[: E.value], d=d[: E.value], label=label, stats=self.mst_stats(), info=self.mst_info())

    def tree_fit(self, parent, length, n=None):
        """tree_fit_host's result, computed on the device from the context's fresh matrix (after dist_matrix, before nj_run); the
        context's matrix is left as it was"""
        n = self.n_total() if n is None else int(n)
        parent, length, m = _tree_args(n, parent, length)
        out, ptrs = _fit_out(max(n, 1))
        _chk(self.L, self.L.dpr_tree_fit(self.h, n, m, _p(parent, c_i32p), _p(length, c_f64p), *ptrs))
        return _fit_result(out)

    def tree_patristic_rows(self, n, parent, length, row0=0, nrows=None):
        """(nrows, n) array of the tree's path lengths between the tips row0 .. row0 + nrows and every tip, through the device's
        lowest-common-ancestor lookup; needs no matrix"""
        nrows = n - row0 if nrows is None else int(nrows)
        parent, length, m = _tree_args(n, parent, length)
        out = np.zeros((max(nrows, 1), n))
        _chk(self.L, self.L.dpr_tree_patristic_rows(self.h, n, m, _p(parent, c_i32p), _p(length, c_f64p), int(row0), nrows, _p(out, c_f64p)))
        return out[:nrows]

    def fit_stats(self):
        """dict(bytes held, allocations so far, launches of the last tree_fit, rows of its lookup table)"""
        out = np.zeros(4, dtype=np.int64)
        _chk(self.L, self.L.dpr_get_fit_stats(self.h, _p(out, c_i64p)))
        return dict(bytes=int(out[0]), allocations=int(out[1]), launches=int(out[2]), levels=int(out[3]))

    def fit_timing(self):
        """(ms of the two passes of the last tree_fit, ms of the NJ row-sum kernel beside them or 0 without set_fit_compare(True))"""
        r, c, b = C.c_double(), C.c_double(), C.c_double()
        _chk(self.L, self.L.dpr_get_fit_timing(self.h, C.byref(r), C.byref(c), C.byref(b)))
        return r.value + c.value, b.value

    def fit_pass_timing(self):
        """(ms of the row pass, ms of the column pass) of the last tree_fit"""
        r, c = C.c_double(), C.c_double()
        _chk(self.L, self.L.dpr_get_fit_timing(self.h, C.byref(r), C.byref(c), None))
        return r.value, c.value

    def set_fit_compare(self, on):
        """time the NJ row-sum kernel over the same fresh matrix after every tree_fit (measurement aid)"""
        _chk(self.L, self.L.dpr_ctx_set_fit_compare(self.h, 1 if on else 0))

    def transfer_taxa(self, n, main_x, main_y, rep_x, rep_y, cutoff_permille=300, phi_sum=None, moved=None, pairs=None):
        """transfer_taxa_host's numbers, computed on the device"""
        (mx, my, rx, ry), phi_sum = _tbe_args(n, main_x, main_y, rep_x, rep_y, phi_sum)
        moved, pairs = _taxa_args(n, moved, pairs)
        _chk(self.L, self.L.dpr_transfer_taxa(self.h, n, _p(mx, c_i32p), _p(my, c_i32p), _p(rx, c_i32p), _p(ry, c_i32p),
                                              cutoff_permille, _p(phi_sum, c_i64p), _p(moved, c_i64p), _p(pairs, c_i64p)))
        return phi_sum, moved, pairs

    def set_tbe_lds(self, nbytes):
        """test hook: LDS budget of transfer_support's tables (0 = its own rule; below one node's table: global memory)"""
        _chk(self.L, self.L.dpr_ctx_set_tbe_lds(self.h, nbytes))

    def comm_sum_i64(self, values):
        """in-place 64-bit integer sum over the context's ranks"""
        a = np.ascontiguousarray(values, dtype=np.int64)
        _chk(self.L, self.L.dpr_comm_sum_i64(self.h, _p(a, c_i64p), len(a)))
        return a

    def msa_counts(self, row):
        u = np.zeros(max(row, 1), dtype=np.int32)
        m = np.zeros(max(row, 1), dtype=np.int32)
        _chk(self.L, self.L.dpr_get_msa_counts(self.h, row, _p(u, c_i32p), _p(m, c_i32p)))
        return u[:row], m[:row]

    def prune_stats(self):
        a = C.c_uint64()
        b = C.c_uint64()
        _chk(self.L, self.L.dpr_get_prune_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def timing(self):
        a = C.c_double()
        b = C.c_double()
        _chk(self.L, self.L.dpr_get_timing(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value
