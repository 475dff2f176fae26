/*
 * dipper_hip.h -- C ABI of the MI355X (gfx950) hot path of the `dipper` phylogeny engine.
 *
 * The reference (TurakhiaLab/DIPPER) has no FFI layer: its hot path is reached through the
 * methods of the structs declared in src/mash_placement.cuh.  Each entry point below names the
 * reference interface it replaces (file:line under /root/reference).  The reference computes one
 * matrix row per kernel launch and crosses the host/device boundary every row and every NJ
 * iteration; this ABI is deliberately coarser (whole matrix / whole run per call).
 *
 * Conventions
 *   - plain C types only; every function returns 0 on success, <0 on error; the message of the
 *     last error of the calling thread is returned by dpr_last_error().
 *   - the caller owns every host buffer; the library owns all device memory of a dpr_ctx.
 *   - one dpr_ctx drives ONE GPU from ONE host thread at a time.  Multi-GPU = one process (and one
 *     ctx) per GPU, joined by dpr_comm_init(); the N x N matrix is then sharded by rows
 *     (block-cyclic, DPR_ROW_BLOCK rows).  The row-sharded NJ loop has three exchange plans
 *     (dpr_ctx_set_nj_exchange): legacy = two RCCL all-gathers per iteration (one record, three column
 *     slices; the default until the others have been validated on a multi-GPU node), peer = ONE
 *     all-gather of the rank records, rows x / y pulled from their owners' memory, mailbox = no
 *     collective at all (records stored straight into every rank's mailbox over xGMI).
 *   - nothing here falls back to the CPU: without a usable gfx950 device dpr_create() fails.
 */
#ifndef DIPPER_HIP_H
#define DIPPER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default)

#define DPR_ABI_VERSION 1
#define DPR_ROW_BLOCK 64 /* rows per ownership block of the sharded matrix */

/* distance sources for dpr_dist_matrix / dpr_place_run */
#define DPR_SRC_MSA 1    /* 4-bit packed aligned sequences, MSADeviceArrays  */
#define DPR_SRC_MASH 2   /* bottom-S sketches,              MashDeviceArrays */
#define DPR_SRC_MATRIX 3 /* PHYLIP lower triangle,          MatrixReader     */

/* distance types of `-d` (src/MSA.cu:81-86) */
#define DPR_DIST_UNCORRECTED 1
#define DPR_DIST_JC 2
#define DPR_DIST_TAJIMANEI 3
#define DPR_DIST_K2P 4
#define DPR_DIST_TAMURA 5
#define DPR_DIST_JINNEI 6
/* protein alignments only (dpr_set_msa_aa; no reference counterpart).  With p = 1 - match / useful over the sites where both
 * sequences hold one of the 20 residues (pairwise deletion), all in fp64 in this operation order:
 *   1 p   2 -0.95 * log(1.0 - p / 0.95)   7 -log(1.0 - p)   8 -log(1.0 - p - 0.2 * p * p)  (Kimura 1983)
 * Types 3-6 are nucleotide models (DPR_ERR_ARG on a protein alignment); 7-8 are DPR_ERR_ARG on a nucleotide alignment. */
#define DPR_DIST_POISSON 7
#define DPR_DIST_KIMURA 8
/* nucleotide alignments only (dpr_set_msa; no reference counterpart; DPR_ERR_ARG on a protein alignment).  For the ordered pair
 * (row a, column b), F[i][j] = the number of sites where a holds base i, b holds base j and both are bases; base order
 * A, C, G, T = 0..3.  All integers: N = sum F, r_i = sum_j F[i][j], c_j = sum_i F[i][j], a_i = r_i + c_i.
 *   9  TN93 (Tamura-Nei 1993): g_i = a_i / (2N), gR = gA + gG, gY = gC + gT, P1 = (F[A][G] + F[G][A]) / N,
 *      P2 = (F[C][T] + F[T][C]) / N, Q = (N - trace F) / N - P1 - P2, k1 = 2 gA gG / gR, k2 = 2 gC gT / gY,
 *      k3 = 2 (gR gY - gA gG gY / gR - gC gT gR / gY),
 *      d = -k1 ln(1 - P1/k1 - Q/(2 gR)) - k2 ln(1 - P2/k2 - Q/(2 gY)) - k3 ln(1 - Q/(2 gR gY));
 *      NaN when N = 0, a_A a_G = 0 or a_C a_T = 0; not finite when a logarithm's argument is <= 0.
 *   10 LogDet (Lockhart 1994): d = -1/4 ln(det F / N^4) - ln 4; det F = 0 with N > 0 gives +inf, det F < 0 or N = 0 NaN.
 *   11 paralinear (Lake 1994): d = -1/4 ln(det F / sqrt(prod_i r_i c_i)); det F < 0 gives NaN, det F = 0 gives +inf when
 *      prod r_i c_i > 0, else NaN.
 * det F is computed exactly in integers, and every value is a function of integers that do not change when a and b swap
 * (a_i, F[i][j] + F[j][i], trace, N, det F, r_i c_i): D[a][b] and D[b][a] are the same bits however they are computed. */
#define DPR_DIST_TN93 9
#define DPR_DIST_LOGDET 10
#define DPR_DIST_PARALINEAR 11

/* error codes */
#define DPR_OK 0
#define DPR_ERR_ARG -1
#define DPR_ERR_HIP -2     /* "Gpu_ERROR: ..." in the reference (e.g. src/neighborJoining.cu:44-55) */
#define DPR_ERR_STATE -3   /* call order violated */
#define DPR_ERR_NOCAND -4  /* no Q candidate below the reference's init value 10000 */
#define DPR_ERR_COMM -5

typedef struct dpr_ctx dpr_ctx;

const char *dpr_last_error(void);
int dpr_abi_version(void);

/* ---- host-only encoders (no GPU needed) ------------------------------------------------------
 * replace fourBitCompressor (src/fourBitCompressor.cpp:5-41) and twoBitCompressor
 * (src/twoBitCompressor.cpp:5-41): out has ceil(len/16) resp. ceil(len/32) words. */
int dpr_pack4(const char *seq, uint64_t len, uint64_t *out);
int dpr_pack2(const char *seq, uint64_t len, uint64_t *out);
/* amino acids (no reference counterpart): out has len bytes; the 20 letters ARNDCQEGHILKMFPSTWYV, in either case, become
 * 0..19 in that order, every other byte (gaps, X, B, Z, J, U, O, *, digits, ...) 255 = not a residue. */
int dpr_pack_aa(const char *seq, uint64_t len, uint8_t *out);

/* ---- host-only sharding helpers (pure functions; used by the N>1 host logic and its CPU tests) */
/* ... and of the ROW-SHARDED EXACT PRUNED NJ (njr.hip; several ranks, dpr_ctx_set_nj_multi_plan(ctx, 3) / DPR_NJ_MULTI=rows, or
 * chosen by itself once two copies of the matrix no longer fit one GPU): north_star's row-block split of the N x N matrix
 * (src/neighborJoining.cu:117-148) under the pruned algorithm.  The position-space matrix (positions = nodes sorted by row sum,
 * per epoch) is dealt in chunks of DPR_NJR_CHUNK positions: chunk k belongs to rank k % world and is that rank's (k / world)-th
 * chunk; the 16 x 512 units, their bounds, tests and scans belong to the owner of their rows. */
#define DPR_NJR_CHUNK 1024
int dpr_njr_owner(int64_t position, int world);              /* rank owning the matrix row of `position`           */
int64_t dpr_njr_local_row(int64_t position, int world);      /* its index in the owner's storage                   */
int64_t dpr_njr_global_pos(int64_t local_row, int rank, int world);   /* inverse                                  */
int64_t dpr_njr_rows_cap(int64_t positions, int world);      /* matrix rows a rank must be able to hold (whole chunks) */
int dpr_shard_owner(int64_t row, int world);                 /* rank owning matrix slot `row`      */
int64_t dpr_shard_local_row(int64_t row, int world);         /* its index in the owner's storage  */
int64_t dpr_shard_rows(int64_t n, int rank, int world);      /* #slots < n owned by `rank`         */
int64_t dpr_shard_global_row(int64_t local, int rank, int world);
/* lexicographic (q, key) minimum over `count` 32-byte records {double q; uint64 key; double d; pad};
 * returns the index of the winner or -1 when no record has key != UINT64_MAX. */
int dpr_record_reduce(const void *records, int count);
/* tie-break key of ordered pair (i,j) at active size n (src/neighborJoining.cu:124-146,214) */
uint64_t dpr_nj_key(int64_t i, int64_t j, int64_t n);

/* ---- context ---------------------------------------------------------------------------------
 * replaces cudaSetDevice(1) (src/tree_generation.cu:240-245; the hard-coded device index is a
 * reference quirk). */
int dpr_create(dpr_ctx **out, int device);
int dpr_destroy(dpr_ctx *ctx);
/* Validation mode of the multi-GPU path: ONE context holds `world` virtual ranks on one device and
 * runs the sharded algorithm (same kernels, same per-rank buffers) with the two per-iteration
 * all-gathers done as device copies instead of RCCL.  Used to prove on a 1-GPU box that the sharded
 * result is bit-identical to the single-rank result. */
int dpr_create_virtual(dpr_ctx **out, int device, int world);
int dpr_device_name(dpr_ctx *ctx, char *buf, int cap);

/* ---- multi-GPU (one process per GPU; RCCL over xGMI).  No reference counterpart (single GPU).
 * rank 0 calls dpr_comm_unique_id, the 128 bytes are broadcast by the launcher (torch.distributed
 * in bench.py), every rank calls dpr_comm_init before any dpr_set_* call. */
int dpr_comm_unique_id(void *out128);
int dpr_comm_init(dpr_ctx *ctx, int rank, int world, const void *id128);
/* 1-rank RCCL round trip on this context's GPU (plumbing check on a single-GPU box) */
int dpr_comm_selftest(dpr_ctx *ctx);
/* Ranks without RCCL: processes whose devices (or ONE shared device -- which RCCL refuses) can map each other's memory.
 * The row-sharded NJ then runs its mailbox plan.  dpr_peer_export allocates this rank's NJ buffers + peer window for
 * n_tips and writes a 192-byte description; the launcher hands every rank all descriptions in rank order
 * (dpr_peer_attach) before dpr_dist_matrix.  With RCCL (dpr_comm_init) the library exchanges them itself. */
int dpr_comm_init_local(dpr_ctx *ctx, int rank, int world);
int dpr_peer_export(dpr_ctx *ctx, int64_t n_tips, void *out192);
int dpr_peer_attach(dpr_ctx *ctx, const void *all192);
/* rank and rank count AS THE COMMUNICATOR REPORTS THEM (ncclCommUserRank / ncclCommCount; for ranks on the window transport of
 * dpr_comm_init_shared: this rank and the number of ranks that have joined the shared region); 0 / 1 without one */
int dpr_comm_info(dpr_ctx *ctx, int *rank, int *nranks);
/* Ranks joined through a SHARED HOST REGION -- what `dipper --gpus G` does (dipper_amd/host/main.cpp forks its ranks around one
 * anonymous shared mapping before any GPU call), and what any launcher can do that hands the G processes of one node the same
 * DPR_COMM_SHARED_BYTES of zero-initialised shared memory (shm_open + mmap).  No reference counterpart: the reference drives one
 * device (src/tree_generation.cu:240-245).  Call after dpr_create, before any dpr_set_* call, on every rank (collective).
 * transport 1 = RCCL: rank 0's ncclUniqueId travels through the region, dpr_comm_init follows -- one rank per GPU;
 * transport 2 = ipc: a device window per rank (DPR_COMM_WINDOW_MB, default 64), mapped by the other ranks through hipIpc; all-gathers
 *   and integer all-reduces run through the windows in chunks between host barriers (synchronous with the host).  The ONLY
 *   transport for ranks that share a device (RCCL refuses them), i.e. for rehearsing every multi-rank path on a single GPU;
 * transport 0 = auto: ipc iff two ranks name the same device (PCI bus id), else RCCL.
 * The region also carries a failure word: a rank that gives up (or the launcher, dpr_shared_abort, when a rank has died) sets it
 * and every wait of every rank ends with DPR_ERR_COMM instead of hanging; DPR_COMM_TIMEOUT_MS (default 600 000) bounds a wait. */
#define DPR_COMM_SHARED_BYTES 65536
int dpr_comm_init_shared(dpr_ctx *ctx, int rank, int world, void *shared, uint64_t bytes, int transport);
/* *transport: 0 = none (one rank / virtual ranks), 1 = RCCL, 2 = device windows over hipIpc, 3 = peers attached by the launcher
 * (dpr_comm_init_local: mailbox NJ only); *collectives: device all-gathers + all-reduces this context has taken part in */
int dpr_comm_stats(dpr_ctx *ctx, int *transport, int64_t *collectives);
/* host-only pieces of that protocol (no GPU needed): the launcher's failure path, and the barrier / 512-byte-per-rank gather the
 * library runs over the region (CPU tests drive them with several processes; *sense is a rank's private word, 0 at the start) */
int dpr_shared_abort(void *shared);
int dpr_shared_failed(const void *shared);
int dpr_shared_barrier(void *shared, int world, uint32_t *sense, int timeout_ms);
int dpr_shared_gather(void *shared, int rank, int world, uint32_t *sense, int timeout_ms, const void *mine, void *all, int bytes);

/* ---- inputs ----------------------------------------------------------------------------------*/
/* MSADeviceArrays::allocateDeviceArrays (src/MSA.cu:14-72): packed4 is [n][ceil(L/16)] words as
 * produced by dpr_pack4; L = length of sequence 0 (src/MSA.cu:19). */
int dpr_set_msa(dpr_ctx *ctx, const uint64_t *packed4, int64_t n, int64_t L);
/* Protein alignment (no reference counterpart): codes is row-major [n][L], one byte per site as dpr_pack_aa writes it; any
 * value >= 20 is not a residue.  Argument limits of dpr_set_msa.  The source stays DPR_SRC_MSA: the alphabet belongs to the
 * uploaded alignment, and each of dpr_set_msa / dpr_set_msa_aa replaces whatever alignment the context held.  Distance types
 * 1, 2, 7, 8 (above).  dpr_msa_resample and dpr_dc_run refuse a protein alignment (DPR_ERR_ARG). */
int dpr_set_msa_aa(dpr_ctx *ctx, const uint8_t *codes, int64_t n, int64_t L);
/* MashDeviceArrays::allocateDeviceArrays (src/mash.cu:14-122): packed2 flat, word_off[i] = first
 * word of sequence i (exclusive scan of ceil(len/32), src/mash.cu:109-119), len[i] in bases. */
int dpr_set_reads(dpr_ctx *ctx, const uint64_t *packed2, const uint64_t *word_off,
                  const uint64_t *len, int64_t n);
/* MatrixReader (src/matrix_reader.cu:15-45): rows concatenated, row i has i entries (i=0..n-1),
 * already parsed with the reference's float rounding by the host reader.  The device copy stays until the next
 * dpr_set_matrix_lower / dpr_destroy, so dpr_dist_matrix(DPR_SRC_MATRIX) and dpr_place_run may be called repeatedly. */
int dpr_set_matrix_lower(dpr_ctx *ctx, const double *rows, int64_t n);

/* ---- Mash sketches: MashDeviceArrays::sketchConstructionOnGpu (src/mash.cu:386-424).
 * S must be 1000 unless the reference quirk of SURVEY 9.8 is lifted; host_sketches (optional)
 * receives [n][S] ascending hashes. */
int dpr_sketch(dpr_ctx *ctx, int k, int S, uint64_t *host_sketches);
/* Read-only test hook: the inverted index over the sketches of the last dpr_sketch (the default pair kernel of every unaligned
 * input) and the constants its kernel is built on.  info[0] built (0 / 1; not built -- DPR_MASH_KERNEL other than auto / index, more
 * than 2^32 sketch values, no memory -- leaves the counts at 0), info[1] chunk_tips (tips per chunk of columns), info[2] chunks,
 * info[3] distinct ((chunk, value) pairs = posting lists), info[4] dense (lists with a block of positions by tip), info[5]
 * dense_min (entries from which a list is dense), info[6] max_sketch (largest sketch size), info[7] beside_task_bound ((chunk, row)
 * tasks of a placement batch above which its launch beside the tree kernels walks them on a bounded grid).  DPR_ERR_ARG on a null
 * context or array, DPR_ERR_STATE before dpr_sketch.  No reference counterpart. */
int dpr_get_mash_index_info(dpr_ctx *ctx, int64_t info[8]);

/* ---- distance matrix: NJDeviceArrays::getDismatrix (src/neighborJoining.cu:35-85) with the row
 * providers MSADeviceArrays/MashDeviceArrays/MatrixReader::distConstructionOnGpu
 * (src/MSA.cu:271-282, src/mash.cu:457-471, src/matrix_reader.cu:23-45), fillDismatrix (:20-32)
 * and calculateU (:94-115).  Builds the (sharded) symmetric fp64 matrix and the row sums U. */
int dpr_dist_matrix(dpr_ctx *ctx, int source, int dist_type, int k);

/* Pay the one-time costs of the process's first hipGraph instantiation (10-30 ms; dpr_nj_run replays graphs) and of its first
 * staged copies between pageable memory and the device (~9 ms each way unless an upload has paid already; the first epoch
 * rebuild of an NJ run reads the row sums back) now -- the CLI calls it from its device thread once the allocations and the
 * upload that waited for the context are done.  No reference counterpart.
 * Threading: like every other entry point it runs on the context's stream and must be the only call on its context (it
 * used to run on a private stream, beside other calls: creating that stream cost 9-16 ms, and the calls beside it waited
 * inside the HIP runtime for as long as they would have waited in a queue). */
int dpr_warm_graphs(dpr_ctx *ctx);

/* Optional: allocate the matrix buffers of a following dpr_dist_matrix over n tips now (cudaMalloc of the n x n matrix
 * in NJDeviceArrays::getDismatrix, src/neighborJoining.cu:41-56); dpr_dist_matrix then finds them in place.  Lets the
 * CLI overlap the allocation with the packing of the input. */
int dpr_reserve_nj(dpr_ctx *ctx, int64_t n);

/* ---- neighbor joining: NJDeviceArrays::findNeighbourJoiningTree (src/neighborJoining.cu:197-249)
 * without the Newick print.  Outputs (host, N-2 entries each): merged matrix slots x<y and the two
 * branch lengths per iteration; *last_d = D[0][1] of the final pair.  max_iters<0 runs all N-2
 * iterations.  The merge log fully determines the tree (realID bookkeeping :233-237 is host work).
 * Returns the number of iterations done (>=0) or an error code. */
int64_t dpr_nj_run(dpr_ctx *ctx, int64_t max_iters, int32_t *merge_x, int32_t *merge_y,
                   double *bl_x, double *bl_y, double *last_d);

/* ---- single Q-argmin at the CURRENT active size (findMinDist + thrust::min_element,
 * src/neighborJoining.cu:117-148,214).  Returns the reference's winning ordered tuple (i,j,q).
 * reps>1 repeats the scan kernel `reps` times (kernel symbol dpr::nj_scan_kernel<true,16,true,false>:
 * the production streaming scan; the first template flag only tags probe launches in profiles,
 * the code is the same) and reports the average duration measured with HIP events on the library's stream;
 * used for the roofline. */
int dpr_argmin_once(dpr_ctx *ctx, int reps, int32_t *out_i, int32_t *out_j, double *out_q,
                    float *out_ms_per_scan);

/* NJ algorithm on a single GPU: 1 = exact pruned scan (default), 0 = full streaming scan every
 * iteration.  Both produce the same merge log bit for bit (tests run both); takes effect at the next
 * dpr_dist_matrix.  Environment DPR_NJ_MODE=stream selects 0 for the CLI. */
int dpr_set_nj_mode(int mode);
/* Several GPUs + pruned scan: every rank keeps the whole matrix and the ranks share the per-iteration unit tests
 * and scans (a unit belongs to one rank for good; one small all-gather of block records per iteration).
 * dpr_set_nj_virtual_shards(w) makes the next dpr_dist_matrix of a single-rank context emulate w such ranks
 * (validation on one GPU; same merge log bit for bit). */
int dpr_set_nj_virtual_shards(int w);
/* Several ranks (dpr_comm_init), pruned NJ: plan 0 = auto (unit-sharded scans + one all-gather per iteration from
 * 65 536 tips on; below that every rank runs the single-GPU plan on its own copy of the matrix -- an iteration is then
 * ~20 us of dependent latency, which a collective per iteration would only lengthen), 1 = always unit-sharded,
 * 2 = never.  Also DPR_NJ_MULTI=auto|shard|solo.  No counterpart in the reference (single GPU,
 * src/tree_generation.cu:240-245).  dpr_nj_is_unit_sharded: what the last dpr_dist_matrix chose. */
int dpr_set_nj_multi_plan(int plan);
int dpr_nj_is_unit_sharded(dpr_ctx *ctx);
/* the multi-rank NJ plan the last dpr_dist_matrix set up, in words ("single rank", "pruned, every rank runs ... (replicas)",
 * "pruned, ... unit tests and scans sharded ...", "streaming, rows sharded ..., exchange ...", "row-sharded pruned NJ ...") */
int dpr_get_nj_multi_info(dpr_ctx *ctx, char *buf, int cap);
/* The NJ plan of a context: one of these kinds, chosen by dpr_nj_plan_resolve and by nothing else. */
#define DPR_NJ_PLAN_SINGLE_STREAM 0 /* one rank, full Q scan every iteration */
#define DPR_NJ_PLAN_SINGLE_PRUNED 1 /* one rank, exact pruned scan (with dpr_set_nj_virtual_shards: emulated unit shards) */
#define DPR_NJ_PLAN_BIONJ 2         /* BIONJ: the streaming loop on this rank's own whole copy, whatever the world */
#define DPR_NJ_PLAN_ROWS_STREAM 3   /* several ranks, rows dealt block-cyclically, streaming (dpr_ctx_set_nj_exchange) */
#define DPR_NJ_PLAN_REPLICAS 4      /* several ranks, each runs the single-GPU pruned plan on its own whole copy */
#define DPR_NJ_PLAN_UNIT_SHARDED 5  /* several ranks, whole copy each, unit tests and scans of an iteration shared */
#define DPR_NJ_PLAN_ROWS_PRUNED 6   /* several ranks, rows dealt, exact pruned scan (njr.hip) */
/* Host-only, pure (no device, no environment): the kind that dpr_dist_matrix sets up for n tips, or DPR_ERR_ARG.  world: ranks
 * of the context; virtual_ranks: they all live in one context (dpr_create_virtual); variant: dpr_ctx_set_nj_variant; pruned:
 * the NJ mode asks for the pruned scan; multi_plan 0..3: dpr_set_nj_multi_plan; virtual_shards >= 1; total_bytes: the device's
 * memory, read by the auto rule of real ranks only.  In this order:
 *   BIONJ                               virtual ranks or virtual shards > 1: DPR_ERR_ARG; else BIONJ, for any world (several real
 *                                       ranks: each keeps its own copy, allocated as rank 0 of 1)
 *   streaming wanted, or n < 3          world 1: SINGLE_STREAM; else ROWS_STREAM, whatever multi_plan says
 *   world 1                             SINGLE_PRUNED (virtual shards are a detail of that plan)
 *   multi_plan 3                        ROWS_PRUNED, virtual or real ranks
 *   virtual ranks, multi_plan 0, 1, 2   ROWS_STREAM, whatever the memory says (a context of virtual ranks keeps no whole copies)
 *   real ranks, multi_plan 1 / 2        UNIT_SHARDED / REPLICAS
 *   real ranks, multi_plan 0            16.0 * n * n > 0.85 * total_bytes (two epoch buffers of a whole copy do not fit):
 *                                       ROWS_PRUNED; else UNIT_SHARDED from 65 536 tips on, REPLICAS below */
int dpr_nj_plan_resolve(int world, int virtual_ranks, int variant, int pruned, int multi_plan, int virtual_shards, int64_t n,
                        uint64_t total_bytes);
/* The three plan knobs above are process-wide DEFAULTS.  Per context (two contexts of one process may run different
 * plans): same meaning, value -1 = follow the process-wide default again; effective at that context's next
 * dpr_dist_matrix. */
int dpr_ctx_set_nj_mode(dpr_ctx *ctx, int mode);
int dpr_ctx_set_nj_multi_plan(dpr_ctx *ctx, int plan);
/* Adaptive plan of the single-rank NJ (default on; DPR_NJ_ADAPTIVE=0 switches it off): the exact pruned scan while its
 * bounds prune; once more than 70 % of an epoch's units are listed per iteration (tie-heavy / arbitrary `-i d` matrices,
 * src/matrix_reader.cu:23-45 feeds NJ anything) the run is handed over to the streaming loop of src/neighborJoining.cu:
 * 117-148,211-243 (dense slot-space matrix, one full Q scan per iteration); pruned epochs are probed again later with a
 * back-off.  Same merge log either way. */
int dpr_ctx_set_nj_adaptive(dpr_ctx *ctx, int on);
int dpr_get_nj_adaptive_stats(dpr_ctx *ctx, int64_t *stream_iterations, int64_t *stream_epochs);
/* Exchange plan of the ROW-SHARDED streaming NJ loop (several ranks, DPR_NJ_MODE=stream / dpr_ctx_set_nj_mode(ctx, 0);
 * replaces src/neighborJoining.cu:211-243): 0 = legacy (4 launches + 2 all-gathers per iteration; the DEFAULT since round 4:
 * the other two have only run on one device so far), 1 = peer (2 launches + ONE all-gather of the rank records; rows x / y are
 * pulled from their owners' memory), 2 = mailbox (2 launches, no collective: the records go straight into every rank's
 * mailbox); -1 = DPR_NJ_EXCHANGE (legacy | peer | mailbox) / default.
 * A plan that cannot be set up on every rank falls back to 0 on all ranks together (note in dpr_get_nj_exchange_info).
 * Plans 1 and 2 check themselves every iteration: each rank's record carries the bits of the row sum it derived from the rows
 * it pulled (replicated state: identical on every rank by construction) and its status; a differing word, a record of another
 * iteration or a poll that times out ends dpr_nj_run with DPR_ERR_COMM on every rank. */
int dpr_ctx_set_nj_exchange(dpr_ctx *ctx, int plan);
/* test hook of that cross-check (no counterpart in the reference): rank `rank` uses a wrong value for one element of a row it
 * pulled at iteration `iteration`; (-1, -1) = off.  Effective for the context's following dpr_nj_run calls. */
int dpr_ctx_set_debug_fault(dpr_ctx *ctx, int64_t iteration, int rank);
/* what the last dpr_dist_matrix set up (*active_plan, note) and what the last dpr_nj_run enqueued on this rank */
int dpr_get_nj_exchange_info(dpr_ctx *ctx, int *active_plan, int64_t *launches, int64_t *collectives, char *note, int cap);
/* bound of one mailbox / barrier poll in ms (default 2000): a rank whose record does not arrive ends the run with DPR_ERR_COMM */
int dpr_ctx_set_poll_limit_ms(dpr_ctx *ctx, int ms);
int dpr_ctx_set_nj_virtual_shards(dpr_ctx *ctx, int w);
/* Tree-building algorithm of a context: variant 0 = NJ (Saitou & Nei; default), 1 = BIONJ (Gascuel 1997: NJ's pair selection
 * and branch lengths; the new node's distances are a variance-weighted mean with one weight lambda per merge).  Takes effect
 * at the context's next dpr_dist_matrix / dpr_reserve_nj.  A BIONJ context always runs the single-rank streaming plan (one
 * full Q scan per iteration) whatever dpr_set_nj_mode, DPR_NJ_MODE, the adaptive switch and the multi-rank plans say; with
 * several real ranks every rank builds the whole tree on its own copy of the matrix, no collective.  A context of virtual
 * ranks (dpr_create_virtual) or with dpr_set_nj_virtual_shards > 1 gets DPR_ERR_ARG from dpr_dist_matrix.  dpr_nj_run is
 * unchanged: merge log, partial runs and resuming as for NJ.
 *
 * Arithmetic contract of BIONJ (fp64, exactly this order of operations, no contraction; the device loop and
 * dpr_nj_variant_host below produce the same bits):
 *   State: as the streaming NJ, in slot space -- D, U, Ur and the keys -- plus V with D's layout and row stride, a copy of D
 *     (pads included) once the distance source has filled D.
 *   Selection: the Q scan and the reduction of its records, tie-break key and the no-candidate rule q == 10000.0 as for NJ.
 *   Winner x < y, d = D[y][x], last slot n - 1, r = (double)(n - 2).
 *   bx0 = (d + U[x]/r - U[y]/r) * 0.5;  by0 = d - bx0.  The merge log receives the clamped lengths exactly as for NJ; the
 *     update uses the unclamped bx0, by0.
 *   vxy = V[y][x];  s = sum over the slots k < n of t_k, t_k = V[y][k] - V[x][k] for k != x, y and 0.0 for k = x, y, in the
 *     canonical order of U[x]: pairwise tree over each chunk of 256 slots, then the chunk partials folded by 256 classes
 *     (ascending) and combined by the same tree.
 *   lam = 0.5 + s / (2.0 * r * vxy);  vxy == 0.0 or lam != lam: lam = 0.5;  otherwise clamped to [0.0, 1.0].
 *   For every slot i < n, i not x or y:
 *     a = D[x][i] - bx0;  b = D[y][i] - by0;  val = b + lam * (a - b);
 *     vnew = V[y][i] + lam * (V[x][i] - V[y][i]) - (lam * (1.0 - lam)) * vxy;
 *     U[i] = U[i] + (-D[x][i] - D[y][i] + val).
 *   Slot moves as for NJ: the new node takes slot x (row and column: val in D, vnew in V), slot n - 1 moves to y (V moves
 *   exactly as D does); U[x] = canonical sum of the chunk partials of val. */
int dpr_ctx_set_nj_variant(dpr_ctx *ctx, int variant);
/* lambda of the iterations done since the last dpr_dist_matrix of a BIONJ context: out[0 .. *count), *count <= n_total - 2 */
int dpr_get_nj_lambda(dpr_ctx *ctx, double *out /* n_total-2 */, int64_t *count);
/* Host-only restatement of the whole loop under the contract above (no GPU; the reference of the tests): selection with
 * dpr_nj_key, the canonical initial row sums, the update.  variant 0: NJ's val = (dxi + dyi - d) * 0.5 (no V, no lambda).
 * lower_rows: the strict lower triangle row by row (row i has i entries), as dpr_set_matrix_lower takes it.  Returns the
 * iterations done: min(n - 2, max_iters) (max_iters < 0: all), fewer when an iteration finds no candidate (the loop ends
 * there; the log up to it is valid), or DPR_ERR_ARG.  last_d is written when two slots remain.  lambda may be NULL. */
int64_t dpr_nj_variant_host(int variant, const double *lower_rows, int64_t n, int64_t max_iters,
                            int32_t *merge_x, int32_t *merge_y, double *bl_x, double *bl_y,
                            double *last_d, double *lambda /* may be NULL */);
/* Measurement aid of the pruned NJ loop (bench.py's `timed_kernels` record): stride > 0 makes the following dpr_nj_run
 * calls enqueue their iterations eagerly (no hipGraph replay) with HIP events on the library's stream around the launches
 * of every stride-th iteration; dpr_get_nj_kernel_timing returns the kernels per iteration, the average microseconds per
 * kernel (launch order, up to 4 entries) and the number of sampled iterations; dpr_nj_kernel_name(i) names kernel i. */
int dpr_ctx_set_nj_kernel_timing(dpr_ctx *ctx, int stride);
int dpr_get_nj_kernel_timing(dpr_ctx *ctx, int *kernels, double *us_avg4, int64_t *samples);
const char *dpr_nj_kernel_name(int idx);
/* debug, needs DPR_NJ_PHASES=<iteration>: 2 kernels x 2048 blocks x 8 phase stamps (100 MHz ticks, 0 = none) of that
 * iteration of the last pruned NJ run (profiles/nj_phases.py) */
int dpr_get_nj_phase_stamps(uint64_t *out32768);
/* debug (profiles/njp_list_shape.py): after a dpr_nj_run that stopped early on the default single-GPU plan, the units the next
 * scan would walk -- codes (sub-unit mask << 28 | strip << 18 | row group), *count of them (at most cap copied) -- the number
 * of positions of the current epoch and, if ur != NULL, the row sums U / (n - 2) by position (NaN: dead / in quarantine) */
int dpr_get_njp_list(dpr_ctx *ctx, int32_t *out, int64_t cap, int64_t *count, int64_t *positions, double *ur, int64_t ur_cap);
/* host-only: owner of the 16-row x 512-column unit (strip = column block, group = row group) among `world` ranks
 * when the position space has P positions (units are tested in blocks of one strip x 256 consecutive row groups,
 * strip-major; test block t and its units belong to rank t mod world); -1 if the unit holds no pair of the strict
 * lower triangle */
int dpr_njp_unit_owner(int64_t strip, int64_t group, int64_t P, int world);
/* pruned path: 16x512 units scanned since dpr_dist_matrix, and units of one full scan */
int dpr_get_prune_stats(dpr_ctx *ctx, uint64_t *units_scanned, uint64_t *units_per_full_scan);
/* state of the NJ run after the last dpr_nj_run: iterations done since dpr_dist_matrix and active size -- also after a
 * call that ended with DPR_ERR_NOCAND (the reference's undefined (0,0) merge, src/neighborJoining.cu:134-141,214): the merge
 * log up to there has been copied to the caller's arrays, this says how many entries it holds */
int dpr_get_nj_progress(dpr_ctx *ctx, int64_t *iterations_done, int64_t *active);
/* pruned path, current epoch: positions, row groups per test block, strips per test block, 1 if the large-shape post
 * kernel (njp_post2_kernel) serves it, blocks of the unit scan (tests: which launch shape a run really used) */
int dpr_get_njp_shape(dpr_ctx *ctx, int64_t *positions, int *row_groups, int *strips, int *post2, int *scan_grid);

/* microbenchmark: microseconds per launch of a chain of `nlaunch` trivial dependent kernels of `grid`
 * blocks on the context's stream, eager (0) or hipGraph replay of 128-node chains (1) */
int dpr_launch_bench(dpr_ctx *ctx, int nlaunch, int grid, int use_graph, float *us_per_launch);
/* measurement aid: a background load of `blocks` 64-thread workgroups spinning on FMAs on a stream of its own until
 * dpr_spin_stop (or max_ms at the latest) -- to see whether the latency-bound loops run at reduced clocks on an idle chip */
int dpr_spin_start(dpr_ctx *ctx, int blocks, int max_ms);
int dpr_spin_stop(dpr_ctx *ctx);

/* tuning knobs of the streaming Q-argmin scan (process-wide): rows per work unit (16 or 64; +128 selects the
 * filtered candidate update), non-temporal loads (0/1), grid size (0 = default 2048, <= 8192).  Results never
 * depend on them. */
int dpr_scan_tune(int rows_per_unit, int nontemporal, int grid);

/* calibration: plain streaming read (16 B/lane, optional non-temporal) of `bytes` of the matrix
 * buffer the Q-argmin scans (the position-space matrix in pruned mode); average milliseconds per pass.  Gives the
 * read ceiling the scan is compared with. */
int dpr_bw_probe(dpr_ctx *ctx, int64_t bytes, int nontemporal, int grid, int reps, float *out_ms);

/* ---- test hooks ------------------------------------------------------------------------------*/
int64_t dpr_n_active(dpr_ctx *ctx);
int64_t dpr_n_total(dpr_ctx *ctx);
int dpr_get_matrix_row(dpr_ctx *ctx, int64_t i, double *out /* n_total doubles */);
int dpr_get_row_sums(dpr_ctx *ctx, double *out /* n_total doubles */);
int dpr_get_msa_counts(dpr_ctx *ctx, int64_t row, int32_t *useful, int32_t *match /* row entries */);
/* the distance block tips [row0, row0 + nrows) x tips [0, ncols) as the placement batches, --add and the divide-and-conquer
 * assignment compute it (MSADistConstructionRangeDC, src/divide_and_conquer/msa.cu:321-372, a row per launch there); out
 * (optional): [nrows][ncols], or [ncols][nrows] when transposed; *ms_avg: average duration of `reps` launches (HIP events) */
int dpr_msa_dist_block(dpr_ctx *ctx, int64_t row0, int64_t nrows, int64_t ncols, int dist_type, int transposed, double *out,
                       int reps, float *ms_avg);
/* MurmurHash3 value of every k-mer position of read `seq` (len-k+1 values), sketch kernel's hash path */
int dpr_get_kmer_hashes(dpr_ctx *ctx, int64_t seq, int k, const uint64_t *word_off, const uint64_t *len,
                        uint64_t *out);
/* closest lists (40n ints / doubles, 5 per slot) and per-tip trace (eid, frac, add) of the last
 * dpr_place_run; any pointer may be NULL */
int dpr_get_place_state(dpr_ctx *ctx, int32_t *cid, double *cdis, double *trace);
/* phase timings of the last dpr_dist_matrix / dpr_nj_run (or dpr_place_run) in milliseconds (HIP events) */
int dpr_get_timing(dpr_ctx *ctx, double *dist_ms, double *nj_ms);

/* ---- k-closest placement: KPlacementDeviceArrays::{allocateDeviceArrays,findPlacementTree,
 * addQuery} (src/placement_close_k.cu:15-68,646-854,858-990).  Adjacency arrays are in/out host
 * buffers of sizes head[2n], e/nxt/belong[8n], len[8n]; first = 2 builds from scratch, first = m
 * expects the imported backbone (initializeDeviceArrays :126-264) in the arrays. */
int dpr_place_run(dpr_ctx *ctx, int source, int dist_type, int k, int64_t first, int64_t n,
                  int32_t *head, int32_t *e, int32_t *nxt, int32_t *belong, double *len);

/* distance and tree part of the last dpr_place_run in milliseconds (the reference prints them as "Distance Operation
 * Time" / "Tree Operation Time", src/placement_close_k.cu:852-853,985-986).  The two add up to the run.  Without
 * overlap dist_ms is the HIP-event time of the distance batches.  Mash input computes the rows of the next batch on a
 * second stream beside the tree kernels: dist_ms is then the time the tree stream WAITED for distance rows (the
 * non-overlapped remainder), not the batches' own duration -- that one is dpr_get_place_overlap's dist_busy_ms */
int dpr_get_place_timing(dpr_ctx *ctx, double *dist_ms, double *tree_ms);
/* *overlapped = 1 if the last placement run computed its distance rows beside the tree kernels; *dist_busy_ms = time the
 * distance batches were in flight then (concurrent with tree work: not a summand of the wall time); 0 / 0.0 otherwise */
int dpr_get_place_overlap(dpr_ctx *ctx, int *overlapped, double *dist_busy_ms);
/* The overlap decision is taken per batch of distance rows (1 024 tips for Mash input): a batch is produced beside the tree
 * kernels of the previous one only while its distance part is the shorter of the two (src/placement_close_k.cu:756-851 computes
 * one row per tip, serially).  *batches / *overlapped_batches of the last placement run.  DPR_PLACE_NO_OVERLAP=1: never,
 * DPR_PLACE_OVERLAP_ALWAYS=1: round 3's policy (every batch).  Results do not depend on it. */
int dpr_get_place_policy(dpr_ctx *ctx, int64_t *batches, int64_t *overlapped_batches);
/* Host-only, pure (no device, no environment): the per-batch overlap policy of dpr_place_run (csrc/place_policy.hpp) run over a
 * described placement of tips [first, last).  world: real ranks; window_transport: they are joined by dpr_comm_init_shared (no
 * RCCL communicator); no_overlap: DPR_PLACE_NO_OVERLAP is set; multi_min: first tip of the four-tip launches
 * (DPR_PLACE_MULTI_MIN, default 150 000); batch_rows: DPR_PLACE_BATCH, outside [16, 65536] = the source's default R (1024 for
 * Mash, 256 otherwise).  Batch b is [i0, i0 + nr), i0 = first + b * R; tree_ms[b] and dist_alone_ms[b] are what the event pairs
 * around its tree kernels and -- were its rows produced alone on the main stream -- around its rows would report.
 * `batches` must be ceil((last - first) / R).  beside[b] = 1 if batch b is produced beside batch b - 1's tree kernels.  The rule:
 *   fixed for a run     allowed = Mash source, no_overlap unset, not (world > 1 on the window transport, whose all-gather is
 *                       synchronous with the host); always = allowed and world > 1
 *   pairs(i0, nr)       nr * (i0 + 0.5 * (nr - 1))
 *   learned             tree_ms_per_tip = -1 and pairs_per_ms = 4.5e6 at the start.  Observing a finished batch:
 *                       tree_ms_per_tip = tree_ms / nr / (its tree kernels ran alone ? 1 : 1.4); if its rows were produced alone,
 *                       its pairs are >= 5e7 and dist_alone_ms > 0: pairs_per_ms = pairs / dist_alone_ms.  In order, latest wins.
 *   successor [j0, j0 + nr2) of batch [i0, i0 + nr), j0 = i0 + R:
 *                       not allowed, or j0 >= last: no.  always, or i0 + nr <= multi_min: yes.  Otherwise every batch before
 *                       the current one is observed, est = pairs(j0, nr2) / pairs_per_ms, and the answer is
 *                       est < tree_ms_per_tip * nr once tree_ms_per_tip > 0, est < 1.0 before that.
 * Only the last case reads timings (there dpr_place_run's host waits for batch b - 1, and no further). */
int dpr_place_policy_run(int source, int world, int window_transport, int no_overlap, int64_t multi_min, int64_t first, int64_t last,
                         int64_t batch_rows, const double *tree_ms, const double *dist_alone_ms, int64_t batches, int32_t *beside);

/* Per placed tip of the last placement run: slots its closest-list walk reached (updateClosestNodes, src/placement_close_k.cu:
 * 86-124) beyond the two rounds applied with the split; negative = -(reached + 1): the walk of a node of degree > 3 (imported
 * backbones).  The update launch of a tip grows with it (64 queue entries per round trip): the outliers of those launches.
 * stats6: tips whose walk left the 2 048-entry LDS queue, largest walk, sum, tips on the degree > 3 walk, and -- the second kind of
 * outlier, four-tip launches only -- tips for which the launch evaluated EVERY slot itself because the set of slots changed by the
 * launch's earlier tips overflowed / because more than 128 blocks had to be re-scanned.  DPR_LOG=place prints the six numbers. */
int dpr_get_place_walks(dpr_ctx *ctx, int32_t *reached /* n entries or NULL */, int64_t *stats6);

/* ---- exact placement mode: PlacementDeviceArrays::{allocateDeviceArrays,findPlacementTree}
 * (src/placement.cu:17-117,508-789), reached in the reference through `-m 0` with 30000 <= n < 1000000
 * (SURVEY 9.2).  Same inputs/outputs as dpr_place_run with first = 2; per tip the per-slot bounds come
 * from an exact bottom-up / top-down pass over the whole tree instead of the K = 5 closest lists. */
int dpr_place_exact_run(dpr_ctx *ctx, int source, int dist_type, int k, int64_t n, int32_t *head, int32_t *e,
                        int32_t *nxt, int32_t *belong, double *len);
/* test hook: reverse-slot array (8n) and node depths below node n (2n) of the last dpr_place_exact_run */
int dpr_get_exact_state(dpr_ctx *ctx, int32_t *rev, int32_t *dep);

/* ---- divide-and-conquer mode: KPlacementDeviceArraysDC::{findBackboneTreeDC, findClustersDC,
 * findClusterTreeDC} (src/divide_and_conquer/placement_close_k.cu:731-935, 937-1113, 1251-1535) with the
 * DC row providers MashDeviceArraysDC / MSADeviceArraysDC (src/divide_and_conquer/mash.cu:453-755,
 * msa.cu:219-504); dispatch at src/tree_generation.cu:422-449,541-575 (`-m 3` or n >= 1 000 000).
 * Tips [0, backbone) form the backbone (the CLI passes n/20, src/tree_generation.cu:425,545), every
 * other tip is assigned to a backbone edge and placed inside that edge's cluster.  Unlike the
 * reference nothing is staged through host memory: all planes / sketches stay in HBM.
 * Adjacency outputs as dpr_place_run (internal node ids start at n; root-side node n);
 * cluster_id (optional, n entries): -1 for backbone tips, else the backbone slot of the tip's cluster.
 * flags: DPR_DC_EXACT_LAST computes the distance of a query to the LAST backbone tip also for aligned
 * input (the reference's kernel stops one short, src/divide_and_conquer/msa.cu:331, and scans a 0.0;
 * that behaviour is the default so that results match the reference). */
#define DPR_DC_EXACT_LAST 1
/* Multi-GPU: after dpr_comm_init every rank calls dpr_dc_run with the same (replicated) inputs; the
 * backbone is built identically on every rank, the query tips and the clusters are shared out, cluster ids
 * and the state changes are summed over RCCL (two all-reduces per run), and every rank returns the full
 * tree.  DPR_DC_VIRTUAL_RANKS(w) emulates w ranks one after the other on a single GPU (validation of the
 * sharding and of the merge; same result as w = 1, bit for bit). */
#define DPR_DC_VIRTUAL_RANKS(w) (((w) & 0xff) << 8)
int dpr_dc_run(dpr_ctx *ctx, int source, int dist_type, int k, int64_t n, int64_t backbone, int flags,
               int32_t *head, int32_t *e, int32_t *nxt, int32_t *belong, double *len, int32_t *cluster_id);
/* host-only helpers of the multi-GPU split (pure functions; used by dpr_dc_run itself and by the CPU tests):
 * share of the query tips [backbone, n) of `rank` (contiguous, multiples of 256 tips) ... */
int dpr_dc_query_share(int64_t n, int64_t backbone, int rank, int world, int64_t *q0, int64_t *q1);
/* ... and the owner of every cluster: sizes[] in the order dpr_dc_run builds them (descending, ties by
 * ascending slot); largest first onto the least-loaded rank (load = m * (m + 20)), ties to the lowest rank */
int dpr_dc_deal_clusters(const int64_t *sizes_desc, int64_t count, int world, int32_t *owner);
/* counts: clusters, largest cluster, in-cluster pair distances, memory groups, pair jobs;
 * phase_ms: backbone tree, cluster assignment, cluster trees (HIP events) */
int dpr_get_dc_stats(dpr_ctx *ctx, int64_t *counts5, double *phase_ms3);
/* read-only test hook: the assignment table that the last dpr_dc_run built over its backbone (the table itself is freed with the
 * run).  out4[0] entries (eligible backbone slots, 2 * backbone - 2), out4[1] chunks of the assignment scan, out4[2] most entries
 * in one chunk (at most 64), out4[3] most distinct backbone tips named by one chunk's closest lists (at most 48).  Zeros before
 * the first dpr_dc_run of the context; DPR_ERR_ARG on a null context or array.  No reference counterpart. */
int dpr_get_dc_table_stats(dpr_ctx *ctx, int64_t out4[4]);

/* ---- independent placement of queries on a FIXED backbone (no reference counterpart: addQuery, src/placement_close_k.cu:
 * 858-990, inserts the queries one after the other; findClustersDC, src/divide_and_conquer/placement_close_k.cu:937-1113,
 * scores them independently but keeps the edge only).  Tips [0, m) are the backbone, tips [m, n) the queries, as for
 * dpr_place_run with first = m; the backbone is a rooted binary tree in the adjacency form of initializeDeviceArrays
 * (src/placement_close_k.cu:126-264): edge k = the k-th non-root node in post-order owns slot 2k (child to parent) and 2k + 1.
 * Every eligible slot s (belong[s] >= e[s]: one per undirected edge) gets, by the arithmetic of calculateBranchLength
 * (src/placement_close_k.cu:309-358) over the backbone's closest lists, the pendant length `add` and the position `frac` =
 * distance of the attachment point from node belong[s].  The placement of a query is the eligible slot with the smallest
 * (add, slot); ineligible slots take no part (no "add = 2" default tuple), add is never NaN.  Where add < 2 it is what
 * dpr_place_run would do for that query were it the first one added.  The backbone is never modified; no query influences another.
 * For aligned input the distances to ALL m backbone tips are computed (dpr_dc_run's default stops one short, as the reference). */
/* Imports the backbone (host arrays sized as for dpr_place_run, only read), builds its closest lists and the edge table, and
 * keeps them in the context until the next dpr_place_fixed_set, any of dpr_place_run / dpr_place_exact_run / dpr_dc_run
 * (they rebuild the placement state), or dpr_destroy.  3 <= m < n; a backbone with an unused slot below 4m - 4 (polytomy)
 * is DPR_ERR_ARG, as for dpr_place_run. */
int dpr_place_fixed_set(dpr_ctx *ctx, int64_t m, int64_t n, const int32_t *head, const int32_t *e, const int32_t *nxt,
                        const int32_t *belong, const double *len);
/* Places all queries [m, n) from the context's CURRENT input: the MSA planes as dpr_set_msa / dpr_msa_resample left them
 * (DPR_SRC_MSA), or the sketches (DPR_SRC_MASH, k = the sketch k).  slot / frac / add receive n - m entries each, query m + i
 * at index i.  Queries go through in batches sized as dpr_dc_run sizes them.  Several ranks (dpr_comm_init*): contiguous query
 * shares as dpr_dc_query_share, the results all-gathered, every rank returns everything.  A second call reuses every
 * allocation.  DPR_ERR_STATE without a valid dpr_place_fixed_set.  DPR_PFIX_CARRY=1 (A/B aid): the scan carries the position
 * through its loop instead of the reduce step evaluating the winning entry again -- same bits. */
int dpr_place_fixed_run(dpr_ctx *ctx, int source, int dist_type, int k, int32_t *slot, double *frac, double *add);
/* test hook: queries per batch of dpr_place_fixed_run (batch boundaries with a few dozen queries); 0 = dpr_dc_run's rule */
int dpr_ctx_set_place_fixed_batch(dpr_ctx *ctx, int64_t queries);
/* distance blocks / scan + reduce of the last dpr_place_fixed_run in milliseconds (HIP events, summed over the batches) */
int dpr_get_place_fixed_timing(dpr_ctx *ctx, double *dist_ms, double *scan_ms);

/* ---- complete and partial deletion of gappy alignment sites (no reference counterpart) -------------------------------------
 * A sequence HOLDS A SYMBOL at column c when its not-a-base / not-a-residue plane bit is 0 there: nucleotides, one of A, C, G,
 * T/U as dpr_pack4 codes them; protein, one of the 20 residues as dpr_pack_aa codes them.  cov[c], 0 <= c < L, is the number of
 * the n sequences that hold a symbol at c.  With a threshold permille in 1 .. 1000 column c is KEPT iff
 *   1000 * cov[c] >= permille * n      (64-bit integers: a tie is kept)
 * so permille = 1000 is complete deletion, and permille = 1 drops only the columns in which no sequence holds a symbol as long
 * as n <= 1000 (of 30 000 sequences it asks for 30).  The filtered alignment is the kept columns in ascending order; L' is
 * their number.
 * Equivalence: after a successful filter the context is indistinguishable, bit for bit, from a fresh one that uploaded the
 * host-filtered alignment with dpr_set_msa / dpr_set_msa_aa -- the planes with their padding, the per-sequence stage bits and
 * counts, the distance table (full table or band by L', not L), hence dpr_get_msa_counts, every dpr_dist_matrix /
 * dpr_msa_dist_block type, and dpr_msa_resample(seed, r) for nucleotides, whose column draws are a function of L'.
 * The filter is one-way: the uploaded alignment is not kept; a new dpr_set_msa / dpr_set_msa_aa replaces the filtered one. */
/* cov[] (L entries) of the context's current alignment */
int dpr_get_msa_site_coverage(dpr_ctx *ctx, int32_t *out);
/* Returns L' >= 1, or DPR_ERR_ARG for a permille outside 1 .. 1000 and when no column would be kept (the alignment is then
 * untouched and dpr_last_error names the best coverage seen), DPR_ERR_STATE without an uploaded alignment or while a bootstrap
 * replicate is active.  L' == L rewrites nothing.  Otherwise the planes are rebuilt on the device at L' sites, the bootstrap
 * buffers are released and everything derived from the planes is built again as the uploads build it (DPR_MSA_NO_FAST /
 * DPR_MSA_NO_BAND apply). */
int64_t dpr_msa_filter_sites(dpr_ctx *ctx, int permille);

/* ---- bootstrap support of NJ trees from aligned sequences (no reference counterpart) ---------------------------------------
 * Replicate r (0-based) of an alignment of L sites draws L columns with replacement (uint64 arithmetic, wrapping):
 *   mix64(z) = splitmix64's finaliser; key_r = mix64(seed ^ mix64(r)); column_t = ((mix64(key_r ^ t) >> 32) * L) >> 32,
 *   t = 0 .. L-1; w[c] = #{t : column_t = c}.
 * The replicate alignment is every column c, ascending, repeated w[c] times.  It depends on (seed, r, L) only. */
/* The context's MSA planes become those of replicate `replicate` (>= 0) -- on the device; the uploaded planes stay there --
 * or those of the uploaded alignment again (-1).  Takes effect for dpr_dist_matrix, dpr_msa_dist_block and
 * dpr_get_msa_counts, whose results are then bit for bit those of dpr_set_msa with the replicate alignment.
 * DPR_ERR_STATE without dpr_set_msa; a later dpr_set_msa drops the replicate. */
int dpr_msa_resample(dpr_ctx *ctx, uint64_t seed, int64_t replicate);
/* test hook: w[] of the active replicate as the device computed it (L entries); DPR_ERR_STATE when none is active */
int dpr_get_msa_boot_weights(dpr_ctx *ctx, int32_t *out);
/* host only, no GPU: w[] of replicate `replicate` (L entries), from the same mix64 as the device */
int dpr_msa_boot_weights(uint64_t seed, int64_t replicate, int64_t L, int32_t *out);
/* host only, no GPU: main_* and rep_* are merge logs of dpr_nj_run (n-2 entries each, slots as there; the realID bookkeeping
 * of writeNewickFromMerges names internal node n+k after iteration k).  counts[k] (k < n-2) is incremented when the
 * replicate tree contains the split of the main tree's internal node n+k; entries of nodes whose split is trivial (a side
 * with fewer than 2 tips) are left untouched.  Splits are compared as 128-bit XOR hashes of their side without tip 0. */
int dpr_split_support(int64_t n, const int32_t *main_x, const int32_t *main_y, const int32_t *rep_x, const int32_t *rep_y,
                      int32_t *counts);
/* in-place sum of `count` host integers over the context's ranks (RCCL or the shared region's device windows); nothing
 * to do with one rank */
int dpr_comm_sum_i32(dpr_ctx *ctx, int32_t *host_inout, int64_t count);

/* ---- transfer bootstrap expectation (TBE, Lemoine et al. 2018; no reference counterpart) ---------------------------------
 * Main internal node n+k (merge-log numbering as dpr_split_support) has clade A, p = min(|A|, n - |A|); only nodes with p >= 2
 * are computed.  A replicate tree T* has the clades L_v of all its nodes, leaves included:
 *   h = |A| + |L_v| - 2 |A & L_v|,  delta(A, v) = min(h, n - h),  phi(A, T*) = min_v delta(A, v), in [0, p - 1].
 * Over R replicates with S = sum of phi, den = R (p - 1): the TBE label is (200 (den - S) + den) / (2 den). */
/* On the device (tbe.hip): phi_sum[k] += phi(A_k, replicate) for the nodes with p >= 2; the other entries are left untouched.
 * main_* and rep_* are merge logs of dpr_nj_run (n-2 entries each); a bad log is DPR_ERR_ARG.  The main tree is uploaded when
 * its log differs from the previous call's (once per command); the replicate's DFS intervals are built on the host, O(n). */
int dpr_transfer_support(dpr_ctx *ctx, int64_t n, const int32_t *main_x, const int32_t *main_y, const int32_t *rep_x,
                         const int32_t *rep_y, int64_t *phi_sum);
/* host only, no GPU: the same numbers by a plain restatement (per main node, |A & L_v| bottom-up over the replicate's merge
 * order; host threads) -- the test reference */
int dpr_transfer_support_host(int64_t n, const int32_t *main_x, const int32_t *main_y, const int32_t *rep_x, const int32_t *rep_y,
                              int64_t *phi_sum);
/* Per-taxon transfer index (Lemoine et al. 2018, booster --moved-taxa; no reference counterpart).  The branches are the main
 * nodes with p >= 2, the root's two children naming one branch (both with p >= 2: the larger node number is left out).  A
 * (branch, replicate) pair is counted iff 1000 phi <= cutoff_permille (p - 1), 0 <= cutoff_permille <= 999.  Its closest
 * replicate branch is the internal node v with delta(A, v) = phi whose bipartition has the smallest key (smallest tip index of
 * the side s without tip 0, then |s|); its transfer set is T = A ^ L_v if h <= n - h, else A ^ (all tips - L_v); |T| = phi.
 * phi_sum[k] += phi as dpr_transfer_support; moved[t] += [t in T] over this replicate's counted branches (t = tip index,
 * n entries); *pairs += counted branches.  Bad logs and arguments as dpr_transfer_support; a cutoff outside 0..999 is
 * DPR_ERR_ARG; n <= 3 is a no-op.  The transfer index of tip t is moved[t] / pairs. */
int dpr_transfer_taxa(dpr_ctx *ctx, int64_t n, const int32_t *main_x, const int32_t *main_y, const int32_t *rep_x,
                      const int32_t *rep_y, int cutoff_permille, int64_t *phi_sum, int64_t *moved, int64_t *pairs);
/* host only, no GPU: the same numbers restated without intervals (clade marks and a walk over the closest node's subtree;
 * host threads) -- the test reference */
int dpr_transfer_taxa_host(int64_t n, const int32_t *main_x, const int32_t *main_y, const int32_t *rep_x, const int32_t *rep_y,
                           int cutoff_permille, int64_t *phi_sum, int64_t *moved, int64_t *pairs);
/* test hook: LDS bytes dpr_transfer_support may give one workgroup's tables (16 (n/64 + 1) bytes per main node, up to 8 nodes
 * per workgroup; 0 = its own rule: 64 KiB, or one node up to 159 KiB).  A budget below one node's table puts the tables in
 * global memory. */
int dpr_ctx_set_tbe_lds(dpr_ctx *ctx, int64_t bytes);
/* in-place sum of `count` host 64-bit integers over the context's ranks; nothing to do with one rank */
int dpr_comm_sum_i64(dpr_ctx *ctx, int64_t *host_inout, int64_t count);

/* ---- balanced minimum evolution: NNI refinement of an NJ / BIONJ tree and its balanced branch lengths (Desper & Gascuel 2002;
 * no reference counterpart: the reference stops at the NJ tree) ----------------------------------------------------------------
 * Arithmetic contract (fp64, exactly this order of operations, no contraction; the device and dpr_bme_nni_host produce the same
 * bits).
 * Tree.  Tips are 0 .. n-1; internal node n+k is the node made by merge k of a merge log (the realID bookkeeping of
 *   writeNewickFromMerges), k < n-2; the last two nodes of the log are joined by one edge.  The tree is unrooted; for every
 *   definition it is hung from tip t0 = n-1, which gives parent(v), two children per internal node (c0(v) < c1(v) by id) and
 *   sib(v).  t0 has one neighbour c; t0 counts as a tip that is nobody's ancestor.  height(tip) = 0, height(v) = 1 + max over
 *   the children; rank(v) = (height, id).
 * Averages.  S(u,v) = S(v,u), for u != v where neither is an ancestor of the other: both tips (t0 included): the matrix entry
 *   D[u][v]; otherwise, u being the node of larger rank, S = 0.5 * (S(c0(u),v) + S(c1(u),v)).
 *   W(u,v), for v a proper ancestor of u, v != t0 (the average between the clade of u and everything outside the clade of v):
 *   parent(v) = t0: W = S(u,t0); otherwise W = 0.5 * (S(u,sib(v)) + W(u,parent(v))).
 * Length of the edge above v, p = parent(v):
 *   v = c, children A, B:               0.5 * ((S(A,t0) + S(B,t0)) - S(A,B))       (also the pendant edge of t0)
 *   v a tip, C = sib(v):                0.5 * ((S(v,C) + W(v,p)) - W(C,p))
 *   v internal, A = c0(v), B = c1(v), C = sib(v):
 *                                       0.25 * (((S(A,C) + W(A,p)) + S(B,C)) + W(B,p)) - 0.5 * (S(A,B) + W(C,p))
 *   L = the sum of these lengths over v = 0 .. 2n-3, v != t0, ascending and sequential, on the host from the device's lengths.
 *   Nothing is clamped: balanced lengths can be negative and are written as they are.
 * Candidates.  An internal v with p != t0:  s0 = S(A,B) + W(C,p), s1 = S(A,C) + W(B,p), s2 = W(A,p) + S(B,C),
 *   g1 = 0.25 * (s0 - s1) (move 1 exchanges B and C), g2 = 0.25 * (s0 - s2) (move 2 exchanges A and C).  The candidate move is
 *   1 if g1 >= g2, else 2, g its gain; v is a candidate iff g > 0 (a NaN gain is never one; every comparison as written).
 * Selection.  Candidate v is selected iff no other candidate f has {f, parent(f)} and {v, p} in common and g_f > g_v, or
 *   g_f == g_v and f < v.
 * Round.  All selected moves are applied (they touch disjoint node sets; node ids never change, only parents and children),
 *   the averages are rebuilt, the lengths and L' computed.  L' < L: the round is accepted.  Otherwise it is discarded and, from
 *   the same tree, only the candidate with the greatest (g, then smaller v) is applied -- a fallback, counted whether or not it
 *   is accepted -- and accepted if L' < L; if not, the search ends on the tree it had.  The search also ends when a round has no
 *   candidate, or after max_rounds accepted rounds.  max_rounds = 0: the balanced lengths of the input tree. */
/* On the device (bme.hip).  Reads the context's FRESH matrix -- after dpr_dist_matrix, before any NJ iteration, in whatever
 * layout the context's NJ plan gave it -- else DPR_ERR_STATE.  n < 3, n other than the matrix's, a bad log, several ranks,
 * virtual ranks or virtual shards: DPR_ERR_ARG.  One square fp64 table over the 2n-2 nodes holds S and W (12.8 GB at 20 000
 * tips); one that does not fit the device's free memory is DPR_ERR_ARG with the bytes needed in the message.  The context
 * keeps the table: a later call over no more tips allocates nothing; nothing is allocated after the first evaluation of a call.
 * Non-finite distances are computed with like any other.
 * kids: 2(n-2) entries, the children of node n+k hung from t0; *top = c; len: 2n-2 entries, the edge above every node (len[c]
 * is the whole edge t0 - c, len[t0] = 0); L_rounds (may be NULL): max_rounds+1 entries, L of the input tree and after every
 * accepted round; stats4: accepted rounds, moves applied in them, fallbacks, candidates of the input tree. */
int dpr_bme_nni(dpr_ctx *ctx, int64_t n, const int32_t *merge_x, const int32_t *merge_y, int max_rounds, int32_t *kids, int32_t *top,
                double *len, double *L_rounds, int64_t *stats4);
/* host only, no GPU: the whole loop restated over a table in host memory, rows in rank order -- the reference of the GPU tests.
 * lower_rows: the strict lower triangle row by row, as dpr_set_matrix_lower takes it. */
int dpr_bme_nni_host(const double *lower_rows, int64_t n, const int32_t *merge_x, const int32_t *merge_y, int max_rounds, int32_t *kids,
                     int32_t *top, double *len, double *L_rounds, int64_t *stats4);
/* host only, no GPU (test hook): one evaluation of the tree given as dpr_bme_nni writes it (kids, top): per node (2n-2 entries
 * each) the length of the edge above it, the gain g of its candidate move and that move (1, 2; 0: no candidate, gain is then
 * whatever g came to, 0 for tips and c), and L.  A table that is no binary tree over nodes 0 .. 2n-3 is DPR_ERR_ARG. */
int dpr_bme_eval_host(const double *lower_rows, int64_t n, const int32_t *kids, int32_t top, double *len, double *gain, int32_t *move,
                      double *L);
/* of the last dpr_bme_nni, summed over its evaluations (HIP events): building the table / lengths, gains and their copy back */
int dpr_get_bme_timing(dpr_ctx *ctx, double *table_ms, double *select_ms);
/* out4: bytes of the table the context keeps, device allocations dpr_bme_nni has made for this context so far, and of its last
 * call the kernel launches and the evaluations (table builds) */
int dpr_get_bme_stats(dpr_ctx *ctx, int64_t *out4);

/* ---- balanced minimum evolution: SPR search (subtree pruning and regrafting, the BME search of FastME; an NNI is the case
 * k = 1).  Tree, averages, lengths, L and the acceptance rule are those of the NNI contract above; fp64, exactly this order of
 * operations, no contraction; the device and dpr_bme_spr_host produce the same bits.
 * Pruned subtrees.  X is one side of an edge {x0, q}, q internal: the clade of v (x0 = v, q = parent(v), v not t0, not c), numbered
 *   d = v; or everything outside the clade of an internal v (q = v, x0 = parent(v); for v = c this is the tip t0), numbered
 *   d = (2n-2) + v.  3 (n-2) directed subtrees.
 * Path.  a0 and p_1 are q's other two neighbours (either way round); q, p_1 .. p_k, k >= 1, all p_i internal, leads away from X;
 *   b0 is a neighbour of p_k other than p_(k-1) (q for k = 1), and the last neighbour of p_k is the root of Y_k.  A, B, Y_i are
 *   the subtrees beyond a0, b0 and off p_i; C_k is the subtree at p_k towards p_(k-1).  The move takes q out (a0 joins p_1) and
 *   puts it on the edge {p_k, b0}; the target is named by w, the lower node of that edge (w != t0).  Edges at q and inside X are
 *   no targets.
 * d(P,Q) of two disjoint subtrees is S(u,v) of their clade nodes, or W(u,v) where Q is the outside of the clade of v (outside
 *   the clade of c: the tip t0, S(u,t0)).
 * Gain.  h_0 = 0.5, h_k = 0.5 * h_(k-1) (exact powers of two, 0 from k = 1074 on); U_0 = V_0 = 0;
 *   U_k = U_(k-1) + h_k * (d(X,Y_k) - d(A,Y_k));   V_k = 0.5 * V_(k-1) + 0.25 * d(X,Y_k);
 *   g_k = (((0.5 - h_k) * (d(X,A) - d(X,B)) + (U_k - V_k)) + 0.25 * (d(Y_k,B) + d(C_k,B))) - (0.5 * h_k) * (d(A,B) + d(X,B)).
 *   Non-finite values are computed with like any other; a NaN gain is no target's gain.
 * Best target of X: the greatest gain, then the smaller w, over the targets whose gain is not NaN.  X is a candidate iff that
 *   gain is > 0.
 * Selection.  The candidates in the order (gain descending, d ascending); one is selected iff its node set {x0, a0, q,
 *   p_1 .. p_k, b0} shares no node with that of a candidate selected before it.
 * Round.  All selected moves are applied (node ids never change), the tree is hung from t0 again (c0(v) < c1(v) by id) and
 *   evaluated.  L' < L: accepted.  Otherwise the round is discarded and the first candidate alone is applied -- a fallback,
 *   counted whether or not it is accepted -- and accepted if L' < L; if not, the search ends on the tree it had.  It also ends
 *   with no candidate, or after max_rounds accepted rounds.  max_rounds = 0: the outputs of dpr_bme_nni(.., 0, ..). */
/* On the device.  Preconditions, errors, table and outputs as dpr_bme_nni (the context's table is shared: a call after a
 * dpr_bme_nni over no fewer tips allocates no table); the scan's own buffers -- among them one of traversal stacks sized by the
 * resident scan threads, not by n -- are allocated by the first call and kept.  stats6: accepted rounds, moves applied in them,
 * fallbacks, candidates of the input tree, applied moves with k >= 2, the largest k applied. */
int dpr_bme_spr(dpr_ctx *ctx, int64_t n, const int32_t *merge_x, const int32_t *merge_y, int max_rounds, int32_t *kids, int32_t *top,
                double *len, double *L_rounds, int64_t *stats6);
/* host only, no GPU: the whole loop restated -- the reference of the GPU tests */
int dpr_bme_spr_host(const double *lower_rows, int64_t n, const int32_t *merge_x, const int32_t *merge_y, int max_rounds, int32_t *kids,
                     int32_t *top, double *len, double *L_rounds, int64_t *stats6);
/* host only (test hooks).  One scan of the tree (kids, top): per directed subtree d (2 (2n-2) entries each) the gain, target w
 * and path length k of its best target -- gain 0, w -1, k 0 where d is not prunable or has no target with a gain -- and L. */
int dpr_bme_spr_eval_host(const double *lower_rows, int64_t n, const int32_t *kids, int32_t top, double *best_gain, int32_t *best_w,
                          int32_t *best_k, double *L);
/* the gain and path length of the one move (d, w), NaN included; DPR_ERR_ARG if w is no target of d */
int dpr_bme_spr_gain_host(const double *lower_rows, int64_t n, const int32_t *kids, int32_t top, int64_t d, int32_t w, double *gain,
                          int32_t *k);
/* of the last dpr_bme_spr, summed over its evaluations (HIP events): mirror, scan, best of both sides and their copy back;
 * dpr_get_bme_timing gives the table and the lengths of the same call */
int dpr_get_bme_spr_timing(dpr_ctx *ctx, double *scan_ms);
/* out4: bytes of the traversal stacks, device allocations dpr_bme_spr has made for this context beyond the table's, scan
 * launches of its last call, resident scan threads the stacks are sized for */
int dpr_get_bme_spr_stats(dpr_ctx *ctx, int64_t *out4);

/* ---- UPGMA / WPGMA: average-linkage clustering, the rooted and ultrametric distance method (Sokal & Michener 1958; no reference
 * counterpart: the reference builds unrooted NJ trees only) ---------------------------------------------------------------------
 * Arithmetic contract (fp64, exactly this order of operations, no contraction; the device and dpr_upgma_host produce the same
 * bits).
 * State.  n slots and a symmetric matrix D whose diagonal is never read; sizes s[k] = 1.0 (doubles), heights h[k] = 0.0,
 *   real[k] = k.  Iteration it = 0 .. n-2 works on the m = n - it active slots.
 * Order of values.  key(v) is an unsigned 64-bit integer: all ones for a NaN; otherwise, b being the bits of v with +0.0 taken
 *   for -0.0, ~b if the sign bit is set, else b | 2^63.  So negative < zero < positive finite < +inf < NaN.
 * Selection.  The pair 0 <= i < j < m with the smallest (key(D[j][i]), i, j), compared lexicographically.  A pair always exists
 *   for m >= 2: a run does n - 1 merges whatever the matrix holds, +inf and NaN pairs last.
 * Merge.  x = i, y = j, d = D[y][x]; hnew = 0.5 * d; the log gets merge_x[it] = x, merge_y[it] = y, height[it] = hnew.  The new
 *   node is n + it, its children real[x] and real[y], their branch lengths hnew - h[x] and hnew - h[y] as they come: nothing is
 *   clamped.
 * Update.  For every active k other than x and y, a = D[x][k], b = D[y][k]:
 *   linkage 0 (UPGMA): val = (s[x] * a + s[y] * b) / (s[x] + s[y]);     linkage 1 (WPGMA): val = 0.5 * (a + b);
 *   D[x][k] = D[k][x] = val.  Then s[x] = s[x] + s[y], h[x] = hnew, real[x] = n + it.
 * Slot move (NJ's realID bookkeeping).  If y != m-1, slot m-1 moves to y: row, column, s, h and real.  The first n - 2 log
 *   entries are therefore a merge log as dpr_nj_run writes it (0 <= x < y < n - it) and describe the same unrooted tree; the last
 *   entry is always (0, 1) and makes the root. */
/* On the device (upgma.hip).  Reads the context's FRESH matrix -- after dpr_dist_matrix, before any NJ iteration, in whatever
 * layout the context's NJ plan gave it -- else DPR_ERR_STATE.  n < 2, a linkage other than 0 / 1, several ranks, virtual ranks
 * or virtual shards: DPR_ERR_ARG, and the context stays usable.  Works on a square fp64 copy that the context owns (7.2 GB at
 * 30 000 tips) and frees with itself; one that does not fit the device's free memory is DPR_ERR_ARG with the bytes needed in the
 * message.  A later call over no more tips allocates nothing.  The context's own matrix is left as it was: a dpr_nj_run after
 * this call gives the merge log it would have given without it.  merge_x, merge_y, height: n - 1 entries each.  Returns the
 * merges done, n - 1, or an error code. */
int64_t dpr_upgma_run(dpr_ctx *ctx, int linkage, int32_t *merge_x, int32_t *merge_y, double *height);
/* host only, no GPU: the contract restated naively -- a full scan of the lower triangle per iteration, on purpose not the
 * device's algorithm (a cache of every row's nearest neighbour) -- the reference of the GPU tests.  lower_rows: the strict
 * lower triangle row by row, as dpr_set_matrix_lower takes it.  n < 2, a linkage other than 0 / 1, a null pointer: DPR_ERR_ARG. */
int dpr_upgma_host(const double *lower_rows, int64_t n, int linkage, int32_t *merge_x, int32_t *merge_y, double *height);
/* out4: bytes the context holds for dpr_upgma_run, device allocations it has made for this context so far, and of its last call
 * the kernel launches and the rows scanned again for their nearest neighbour (the first fill of the cache not counted) */
int dpr_get_upgma_stats(dpr_ctx *ctx, int64_t *out4);
/* of the last dpr_upgma_run: its n - 1 iterations (HIP events; the copy of the matrix and the first fill of the cache are outside) */
int dpr_get_upgma_timing(dpr_ctx *ctx, double *loop_ms);

/* ---- Fit of a tree to the distance matrix: residuals of the distances against the tree's path lengths (FastME's explained
 * variance, PHYLIP's sum of squares and average percent standard deviation, the cophenetic correlation, per-taxon residuals) ------
 * The tree as arrays.  m nodes, n + 1 <= m <= 2n - 1, the tips are nodes 0 .. n-1.  parent[m]: the parent of every node, -1 for the
 *   one root; len[m]: the edge above every node (the root's entry is ignored).  Internal nodes have two children or more.  Not a
 *   tree -- no root or several, a tip with children (the root a tip included), a parent outside n .. m-1, an internal node with fewer
 *   than two children, a cycle, a node the root does not reach -- is DPR_ERR_ARG.
 * Arithmetic contract (fp64, exactly this order of operations, no contraction; the device and dpr_tree_fit_host produce the same
 * bits).
 * Depths.  depth[root] = 0, depth[v] = depth[parent[v]] + len[v].
 * Path length.  P_ij = (depth[i] - depth[a]) + (depth[j] - depth[a]), a = lca(i, j).
 * Pairs.  {i, j}, i > j, with D_ij the matrix entry, is COUNTED iff D_ij and P_ij are both finite; otherwise it is skipped, adds to
 *   nothing and is tallied.  e = D - P.  Terms of a counted pair: D, P, D * D, P * P, D * P, e * e, and (e * e) / (D * D) if D > 0
 *   (a counted pair with D <= 0 adds to everything but that last sum and its count N_w).
 * Row part of taxon i, one per sum.  256 accumulators start at +0.0; the term of {i, j}, j < i, is added to accumulator j mod 256, j
 *   ascending; then c[t] = c[t] + c[t + s] for t < s, s = 128, 64 .. 1; the part is c[0].
 * Column part of taxon j, for e * e only.  16 accumulators; the term of {i, j}, i > j, is added to accumulator i mod 16, i ascending;
 *   then c[t] = c[t] + c[t + s] for t < s, s = 8, 4, 2, 1; the part is c[0].
 * Totals.  Every sum starts at +0.0 and adds its row parts over i = 0 .. n-1 ascending.  taxon_ss[t] = row part + column part of
 *   e * e; taxon_pairs[t] the counted pairs that hold t.  The largest |e| over the counted pairs, ties to the smaller i and then the
 *   smaller j.  Nothing depends on a launch geometry; there are no floating-point atomics.
 * sums[16]: 0 N counted pairs, 1 skipped pairs, 2 sum D, 3 sum P, 4 sum D D, 5 sum P P, 6 sum D P, 7 SS = sum e e, 8 WSS =
 *   sum e e / (D D), 9 N_w, 10 max |e| (0 without a counted pair), then the derived figures (dpr_tree_fit_derive): 11 rms =
 *   sqrt(SS / N), 12 relative rms = sqrt(WSS / N_w), 13 explained variance 1 - SS / (sum D D - (sum D * sum D) / N), 14 cophenetic
 *   correlation (N sum D P - sum D sum P) / sqrt((N sum D D - sum D sum D) * (N sum P P - sum P sum P)); a zero denominator
 *   gives NaN; 15 is 0.  worst[2]: the pair (i, j), i > j, of max |e|, or (-1, -1). */
/* On the device (fit.hip).  Reads the context's FRESH matrix as dpr_bme_nni does -- after dpr_dist_matrix, before any NJ iteration,
 * in whatever layout the context's NJ plan gave it -- else DPR_ERR_STATE; the matrix is left as it was.  n other than the matrix's,
 * a malformed tree, several ranks, virtual ranks or virtual shards: DPR_ERR_ARG, and the context stays usable.  lca(i, j) is looked
 * up in a sparse table over the depth-first order of the tips, built on the host and uploaded (4 (n - 1) (floor(log2(n - 1)) + 1)
 * bytes).  The context keeps its buffers: a later call over no more tips allocates nothing.  taxon_ss, taxon_pairs: n entries. */
int dpr_tree_fit(dpr_ctx *ctx, int64_t n, int64_t m, const int32_t *parent, const double *len, double *sums, double *taxon_ss,
                 int64_t *taxon_pairs, int32_t *worst);
/* host only, no GPU: the contract restated with lca(i, j) found by climbing the parent array from both tips -- on purpose not the
 * device's lookup -- the reference of the GPU tests.  lower_rows: the strict lower triangle row by row. */
int dpr_tree_fit_host(const double *lower_rows, int64_t n, int64_t m, const int32_t *parent, const double *len, double *sums,
                      double *taxon_ss, int64_t *taxon_pairs, int32_t *worst);
/* host only: sums[11 .. 15] from sums[0 .. 10] -- the one place the derived figures are computed */
int dpr_tree_fit_derive(double *sums);
/* P[row0 .. row0 + nrows)[0 .. n) into out (nrows * n doubles, host memory), through the device's lookup; the diagonal by the same
 * formula with a = i.  Needs no matrix.  The rows' device buffer is allocated for the call and released with it. */
int dpr_tree_patristic_rows(dpr_ctx *ctx, int64_t n, int64_t m, const int32_t *parent, const double *len, int64_t row0, int64_t nrows,
                            double *out);
/* host only: the trees of the builders as arrays, with the node bookkeeping of the command's Newick writers; all give *m = 2n - 1
 * nodes, the root last; parent, len: 2n - 1 entries.  n < 2, a null pointer, an input that is no log / no tree: DPR_ERR_ARG.
 * from_nj: the log of dpr_nj_run (n - 2 merges; merge it makes node n + it above the nodes of slots x and y); the two nodes left hang
 *   from the root, EACH on a branch of 0.5 * last -- neither child carries the whole of `last`.
 * from_kids: the outputs of dpr_bme_nni / dpr_bme_spr; tip n - 1 and top hang from the root, each on 0.5 * len_in[top].
 * from_upgma: the log of dpr_upgma_run (n - 1 merges; branches h - h[x], h - h[y]); the last merge is the root. */
int dpr_tree_from_nj(int64_t n, const int32_t *merge_x, const int32_t *merge_y, const double *bx, const double *by, double last,
                     int32_t *parent, double *len, int64_t *m);
int dpr_tree_from_kids(int64_t n, const int32_t *kids, int32_t top, const double *len_in, int32_t *parent, double *len, int64_t *m);
int dpr_tree_from_upgma(int64_t n, const int32_t *merge_x, const int32_t *merge_y, const double *height, int32_t *parent, double *len,
                        int64_t *m);
/* out4: bytes the context holds for dpr_tree_fit, device allocations it has made for this context so far, kernel launches of the
 * last call, rows of its sparse table */
int dpr_get_fit_stats(dpr_ctx *ctx, int64_t *out4);
/* of the last dpr_tree_fit: the row pass, the column pass (HIP events; the upload of the tree is outside; any may be NULL).
 * rowsum_ms: when dpr_ctx_set_fit_compare(ctx, 1) was called before, the time of the NJ row-sum kernel over the same fresh matrix,
 * launched once after the two passes into a scratch vector -- the yardstick of tools/fit_bench.py; else 0. */
int dpr_get_fit_timing(dpr_ctx *ctx, double *row_ms, double *col_ms, double *rowsum_ms);
int dpr_ctx_set_fit_compare(dpr_ctx *ctx, int on);

/* ---- Pairs within a distance threshold and the clusters they form (the command's -o p; no reference counterpart) -------------------
 * Contract.  Over the n tips of a source, with D_ij the entry dpr_dist_matrix would give the pair: the pairs are all (i, j), j < i,
 *   with D_ij <= threshold compared in fp64 -- a NaN and +inf are never within it, -inf always is -- ordered by i, then by j; d is
 *   D_ij bit for bit.  The clusters are the connected components of the graph these pairs span (single linkage at the threshold);
 *   label[v] is the smallest tip index of v's component.  Nothing depends on a launch geometry, on block_rows or on the order in which
 *   the device joins components.
 * dpr_pairs_begin starts a stream over the uploaded alignment (DPR_SRC_MSA, dist_type as dpr_dist_matrix takes it), the sketches
 *   (DPR_SRC_MASH, k the sketch k) or the triangle of dpr_set_matrix_lower (DPR_SRC_MATRIX); DPR_ERR_STATE without that input.  A
 *   threshold that is NaN, infinite or negative, a negative block_rows, several ranks, virtual ranks: DPR_ERR_ARG.  A stream still open
 *   on the context is dropped.  block_rows: rows of one block, at most 32 768 and n; 0 = as many as put the block at 1 GiB or less
 *   (8 bytes x block_rows x n rounded up to 16 columns), in whole multiples of 64 rows.
 * Memory.  The n x n matrix is never allocated.  The device holds one block of rows (none for DPR_SRC_MATRIX: the triangle the upload
 *   left is read in place), the pairs of one block (16 bytes each; grown to the largest block met, never beyond block_rows (n - 1)
 *   pairs), 8 (block_rows + 1) bytes of counts and 4 n bytes of parents (4 n more during dpr_pairs_labels): O(block_rows n) + O(n).
 * State.  The context's inputs, its matrix and its NJ state are not touched: a dpr_dist_matrix + dpr_nj_run after a stream gives the
 *   merge log a fresh context gives.
 * dpr_pairs_next computes the next block: the provider's rows [r0, r0 + nr) x columns [0, r0 + nr), a count of the kept entries per
 *   row, an exclusive scan, the ordered write, the union of the block's pairs into the forest.  *i, *j, *d point at *count entries in
 *   pinned host memory the library owns, valid until the next call on the context's stream of pairs (NULL when *count is 0);
 *   *rows_done = r0 + nr.  A block may hold no pair; *count == 0 with *rows_done == n is the end of the stream, and every later call
 *   says the same.  DPR_ERR_STATE before dpr_pairs_begin.
 * dpr_pairs_labels, once rows_done has reached n (DPR_ERR_STATE before): label[n].
 * dpr_pairs_stats: out[0] blocks computed, 1 pairs delivered, and -- 0 until dpr_pairs_labels -- 2 components, 3 members of the
 *   largest, 4 components of one member; 5 the largest number of bytes of device memory the stream held at any time.
 * dpr_pairs_end releases everything the stream holds (also done by dpr_destroy); without a stream it does nothing. */
int dpr_pairs_begin(dpr_ctx *ctx, int source, int dist_type, int k, double threshold, int64_t block_rows);
int dpr_pairs_next(dpr_ctx *ctx, const int32_t **i, const int32_t **j, const double **d, int64_t *count, int64_t *rows_done);
int dpr_pairs_labels(dpr_ctx *ctx, int32_t *label);
int dpr_pairs_stats(dpr_ctx *ctx, int64_t out[6]);
int dpr_pairs_end(dpr_ctx *ctx);
/* of the stream so far (either may be NULL).  ms: summed over its blocks (HIP events) the row provider; count + scan + write +
 * union; the copies of the pairs to the host.  shape: the rows of a block as dpr_pairs_begin settled them, and n. */
int dpr_get_pairs_info(dpr_ctx *ctx, double ms[3], int64_t shape[2]);
/* host only, no GPU: the contract restated as a double loop over the strict lower triangle (lower_rows, row by row, as
 * dpr_set_matrix_lower takes it) and a union-find -- on purpose not the device's algorithm -- the reference of the GPU tests.  The
 * first min(*count, cap) pairs go to i / j / d (which may be NULL when cap is 0), *count is the number found; label may be NULL.
 * n < 2, a bad threshold, a null pointer: DPR_ERR_ARG. */
int dpr_pairs_within_host(const double *lower_rows, int64_t n, double threshold, int32_t *i, int32_t *j, double *d, int64_t cap,
                          int64_t *count, int32_t *label);
/* host only: what labels say.  out3: components, members of the largest, components of one member; rank[n] (may be NULL): the 1-based
 * rank of every tip's component, components ordered by their smallest member.  Labels that are not component minima: DPR_ERR_ARG. */
int dpr_pairs_summary_host(const int32_t *label, int64_t n, int64_t out3[3], int32_t *rank);

/* ---- Each sequence's K nearest neighbours (the command's -o n; no reference counterpart) --------------------------------------------
 * Contract.  Over the n tips of a source, with D_ij the entry dpr_dist_matrix would give the pair (read as a symmetric matrix): the
 *   candidates of row i are the columns j != i whose D_ij is finite -- a NaN, +inf and -inf are never neighbours.  Candidate a comes
 *   before candidate b when d_a < d_b in fp64, or d_a == d_b and j_a < j_b (-0.0 == +0.0: the two tie and the column decides).  Row i's
 *   result is the first min(K, candidates) of that order, in that order; d is D_ij bit for bit (a -0.0 stays -0.0).  The places behind
 *   them, up to K, hold j = -1 and d = the NaN 0x7ff8000000000000; cnt[i] says how many places are real.  1 <= K <= DPR_NEAREST_MAX_K,
 *   n >= 2, one rank.  The answer is a function of the matrix alone: nothing depends on block_rows, on a launch geometry or on the
 *   order in which wavefronts finish.
 * dpr_nearest_begin starts a stream over the uploaded alignment (DPR_SRC_MSA, dist_type as dpr_dist_matrix takes it), the sketches
 *   (DPR_SRC_MASH, k the sketch k) or the triangle of dpr_set_matrix_lower (DPR_SRC_MATRIX); DPR_ERR_STATE without that input.  K
 *   outside 1 .. 256, a negative block_rows, fewer than two tips, several ranks, virtual ranks: DPR_ERR_ARG.  A stream of neighbours
 *   still open on the context is dropped; a stream of pairs (dpr_pairs_*) on the same context is a separate thing and is left alone.
 *   block_rows: as dpr_pairs_begin takes it (at most 32 768 and n; 0 = the rows that put the block at 1 GiB or less, in whole multiples
 *   of 64).
 * Memory.  The n x n matrix is never allocated.  The device holds one block of FULL rows, 8 x block_rows x n bytes (n rounded up to 16
 *   columns; for DPR_SRC_MATRIX too: the block is expanded from the triangle so that one kernel serves every source), and per row of
 *   the block 12 K bytes of results and 8 bytes of counts: O(block_rows n) + O(block_rows K).
 * State.  The context's inputs, its matrix and its NJ state are not touched.
 * dpr_nearest_next computes the next block: rows [*row0, *row0 + *rows) x all n columns by the source's row provider (symmetry is not
 *   exploited), then per row one pass that keeps the K best.  *j and *d point at *rows x K entries (row t of the block at t K), *cnt at
 *   *rows counts, in pinned host memory the library owns, valid until the next call on the context's stream of neighbours.  After the
 *   last block: *rows == 0, *row0 == n, the pointers NULL, and every later call says the same.  DPR_ERR_STATE before dpr_nearest_begin.
 * dpr_nearest_stats: out[0] blocks computed, 1 neighbours delivered (the sum of the counts), 2 rows with fewer than K, 3 rows with
 *   none, 4 the times a row's candidate buffer was cut back to its K best before the end of the row (summed over the rows: a measure
 *   of the work, not part of the answer), 5 the largest number of bytes of device memory the stream held at any time.
 * dpr_nearest_end releases everything the stream holds (also done by dpr_destroy); without a stream it does nothing. */
#define DPR_NEAREST_MAX_K 256
int dpr_nearest_begin(dpr_ctx *ctx, int source, int dist_type, int k, int K, int64_t block_rows);
int dpr_nearest_next(dpr_ctx *ctx, const int32_t **j, const double **d, const int32_t **cnt, int64_t *row0, int64_t *rows);
int dpr_nearest_stats(dpr_ctx *ctx, int64_t out[6]);
int dpr_nearest_end(dpr_ctx *ctx);
/* of the stream so far (either may be NULL).  ms: summed over its blocks (HIP events) the row provider (DPR_SRC_MATRIX: the expansion of
 * the triangle); the select; the copies of the results to the host.  shape: the rows of a block as dpr_nearest_begin settled them, n. */
int dpr_get_nearest_info(dpr_ctx *ctx, double ms[3], int64_t shape[2]);
/* host only, no GPU: the contract restated as a loop over the rows with a partial sort under the order above -- on purpose not the
 * device's algorithm -- the reference of the GPU tests.  lower_rows: the strict lower triangle row by row, as dpr_set_matrix_lower
 * takes it; j, d: n x K entries; cnt: n.  n < 2, K outside 1 .. 256, a null pointer: DPR_ERR_ARG, nothing written. */
int dpr_nearest_host(const double *lower_rows, int64_t n, int K, int32_t *j, double *d, int32_t *cnt);

/* ---- The minimum spanning forest of the distances (the command's -o s; no reference counterpart) -------------------------------------
 * Contract.  Over the n tips of a source, with D_ij the entry dpr_dist_matrix would give the pair (read as a symmetric matrix): a pair
 *   (i, j), i > j, is an edge candidate when D_ij is finite -- a NaN, +inf and -inf make no edge.  key(D) is the bits of D (of +0.0 for
 *   either zero) with the sign bit flipped for D >= 0 and all bits flipped for D < 0, compared unsigned: the order of the finite
 *   distances, negative ones included, -0.0 and +0.0 tying.  The candidates are totally ordered by (key(D_ij), i, j).  The answer is
 *   the Kruskal forest under that strict order: a candidate is an edge exactly when its ends are not connected by smaller candidates.
 *   It is unique: no tolerance, and nothing depends on block_rows, on a launch geometry or on the order in which wavefronts finish.
 *   ei / ej / ed hold the E = n - C edges (C the number of components) ascending in that order, ei > ej, ed the entry bit for bit (a
 *   -0.0 stays -0.0); label[v] is the smallest tip index of v's component, as dpr_pairs_labels gives it.  Cutting the edges at a
 *   threshold T gives the components of dpr_pairs_* at T.
 * dpr_mst_run takes the uploaded alignment (DPR_SRC_MSA, dist_type as dpr_dist_matrix takes it), the sketches (DPR_SRC_MASH, k the sketch
 *   k) or the triangle of dpr_set_matrix_lower (DPR_SRC_MATRIX); DPR_ERR_STATE without that input.  ei, ej, ed: n - 1 places; label: n.
 *   Fewer than two tips, a negative block_rows, a null pointer, several ranks, virtual ranks: DPR_ERR_ARG with nothing written.
 *   block_rows: as dpr_nearest_begin takes it (at most 32 768 and n; 0 = the rows that put the block at 1 GiB or less, in whole multiples
 *   of 64).  The full-row providers are relied on to give D_rc and D_cr the same bits, as dpr_nearest_* relies on them.
 * Algorithm.  Boruvka over streamed blocks of full rows.  A round computes every block (the row provider; DPR_SRC_MATRIX: the expansion
 *   of the triangle), finds per row the smallest (key, column) among the finite entries whose column lies in another component, takes
 *   the minimum per component with integer atomics, emits every component's edge once, joins the components with the union-find of
 *   dpr_pairs_* and tells the host how many edges there are: one synchronisation a round.  The rounds end when nothing was emitted or
 *   one component is left; more than ceil(log2 n) + 1 rounds is DPR_ERR_STATE.  At the end the host sorts the edges and replays them
 *   through a union-find: E != n - C, an edge between tips already joined or labels other than the device's is DPR_ERR_STATE (a source
 *   that is not symmetric would show here); nothing is written then.
 * Memory.  The n x n matrix is never allocated.  The device holds one block of FULL rows, 8 x block_rows x n bytes (n rounded up to 16
 *   columns) and 56 bytes a tip (labels, row and component minima, the edges), all released before the call returns.
 * State.  The context's inputs, its matrix and its NJ state are not touched; open streams of pairs or of neighbours are left alone.
 * dpr_mst_stats, of the last successful dpr_mst_run (DPR_ERR_STATE before): out[0] rounds, 1 blocks computed, 2 edges, 3 components, 4
 *   members of the largest, 5 components of one member, 6 the bytes of device memory the call held, 7 rows walked (rounds x n). */
int dpr_mst_run(dpr_ctx *ctx, int source, int dist_type, int k, int64_t block_rows, int32_t *ei, int32_t *ej, double *ed, int64_t *edges,
                int32_t *label);
int dpr_mst_stats(dpr_ctx *ctx, int64_t out[8]);
/* of the last dpr_mst_run (either may be NULL).  ms: summed over its rounds (HIP events) the row provider (DPR_SRC_MATRIX: the expansion
 * of the triangle); the row minimum; the per-round component work (component minimum, emit) and the copy of the count.  shape: the rows
 * of a block as the call settled them, n. */
int dpr_get_mst_info(dpr_ctx *ctx, double ms[3], int64_t shape[2]);
/* host only, no GPU: Kruskal -- every candidate sorted under the order, then a union-find -- on purpose not the device's algorithm; the
 * reference of the GPU tests.  lower_rows: the strict lower triangle row by row, as dpr_set_matrix_lower takes it.  n < 2, a null
 * pointer: DPR_ERR_ARG, nothing written. */
int dpr_mst_host(const double *lower_rows, int64_t n, int32_t *ei, int32_t *ej, double *ed, int64_t *edges, int32_t *label);
/* host only: the single-linkage dendrogram of a CONNECTED forest (edges == n - 1, in the contract's order; else DPR_ERR_ARG) as a merge
 * log in the slot convention of dpr_upgma_run: merge t joins the components of edge t at height 0.5 * ed[t].  n - 1 entries each;
 * dpr_tree_from_upgma and the command's UPGMA Newick writer take the log as it is. */
int dpr_mst_dendrogram_host(int64_t n, const int32_t *ei, const int32_t *ej, const double *ed, int64_t edges, int32_t *merge_x,
                            int32_t *merge_y, double *height);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* DIPPER_HIP_H */
