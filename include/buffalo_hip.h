/*
 * buffalo_hip.h -- C ABI of libbuffalo_hip.so, the MI355X (gfx950) backend for buffalo's
 * ALS / BPRMF / WARP training inner loops.
 *
 * Drop-in boundary: every object below replaces one C++ class that buffalo's Cython bindings wrap
 * (paths relative to the kakao/buffalo tree):
 *
 *   bfh_bpr_*   <->  cuda_bpr::CuBPR     include/buffalo/cuda/bpr/bpr.hpp:29-45
 *                    bound by CyBPR      buffalo/algo/cuda/_bpr.pyx:13-80
 *                    (CPU twin bpr::CBPRMF include/buffalo/algo_impl/bpr/bpr.hpp:21-58,
 *                     whose numerics this backend follows: lib/algo_impl/bpr/bpr.cc:72-188)
 *   bfh_warp_*  <->  warp::CWARP         include/buffalo/algo_impl/warp/warp.hpp:20-67
 *                    bound by CyWARP     buffalo/algo/_warp.pyx; accelerator scaffold
 *                    buffalo/algo/warp.py:212-234 (the reference has no GPU WARP)
 *   bfh_als_*   <->  cuda_als::CuALS     include/buffalo/cuda/als/als.hpp:20-35
 *                    bound by CyALS      buffalo/algo/cuda/_als.pyx:13-67
 *                    (numerics: als::CALS lib/algo_impl/als/als.cc:86-358)
 *
 * Conventions
 *   - Plain C types only. All array arguments are HOST pointers owned by the caller (numpy memory
 *     in buffalo); the backend keeps the factor pointers and writes results back into them exactly
 *     where the reference's CUDA backend does (bpr.cu:334-336, als.cu:403).
 *   - Factor matrices are C-contiguous float32 [rows, vdim], vdim = ceil(d/32)*32, pad columns zero
 *     (buffalo/algo/bpr.py:196-204, als.py:146-152).
 *   - `indptr` is int64[rows] of row END offsets without a leading zero; `keys` / `vals` hold only the
 *     current chunk, shifted by indptr[start_x-1] (buffalo/data/buffered_data.py:99-118).
 *   - Return value: BFH_OK (0) on success, a negative bfh_status on failure with the message
 *     available from bfh_last_error(handle).  `*_init` follows the reference's bool contract:
 *     1 = options parsed, 0 = file missing / invalid JSON (bpr.cu:245, _bpr.pyx:35).
 *   - Calls are synchronous (device idle on return), like the reference (bpr.cu:412,427).
 *   - One handle drives one GPU (the current HIP device at *_create, or bfh_*_set_device).  Every kind takes bfh_*_set_device to any
 *     device until its first allocation and to the device it lives on ever after; any other device is refused (create a new handle).
 */
#ifndef BUFFALO_HIP_H_
#define BUFFALO_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    BFH_OK = 0,
    BFH_ERR_INVALID = -1,   /* bad argument / call order */
    BFH_ERR_HIP = -2,       /* a HIP runtime call or kernel failed */
    BFH_ERR_UNSUPPORTED = -3,
    BFH_ERR_NOMEM = -4
} bfh_status;

/* Kernel-level statistics, cumulative since the last bfh_*_reset_stats. */
typedef struct {
    int64_t samples;          /* (u,pos[,neg]) updates processed                                */
    int64_t scored_negatives; /* WARP: negatives actually scored (sum of T)           */
    int64_t accepted;         /* WARP: positives for which a violator was found                  */
    int64_t launches;         /* launches of the dominant kernel                                  */
    double kernel_ms;         /* HIP-event time of the dominant kernel, summed over launches      */
    double optimizer_ms;      /* HIP-event time of the epoch-end optimizer kernels                */
    double aux_ms;            /* everything else the backend launched (precompute, loss, ...)     */
    double h2d_bytes, d2h_bytes;
    int64_t merges;           /* BPRMF policy 2: reconciliations of the per-XCD item-factor replicas */
    int64_t exchanges;        /* multi-GPU: all-reduce exchange points (bfh_*_set_comm) */
    int64_t loaded_rows;      /* WARP: candidate rows fetched by the trial loop (scored + speculated), for the byte model */
    double exchange_kernel_ms; /* multi-GPU: HIP-event time of the delta / weight / apply kernels around the all-reduces */
    double allreduce_ms;       /* multi-GPU: time of the all-reduces on the stream they ran on (blocking exchanges; an exchange
                                  still in flight when the call returns is not counted) */
} bfh_stats;

const char* bfh_version(void);
/* sizeof(bfh_stats) of THIS library: the struct grows at its end between versions, a caller built against an older header can check that
 * its buffer is large enough before calling bfh_*_get_stats (which writes the whole struct). */
size_t bfh_stats_size(void);
/* Message of the last failure on `handle` (any bfh object), or of the last failed *_create when
 * handle is NULL.  Never returns NULL. */
const char* bfh_last_error(const void* handle);
int bfh_device_count(void);

/* ------------------------------------------------------------------------------------------------
 * BPRMF   (CuBPR: include/buffalo/cuda/bpr/bpr.hpp:29-45)
 * ---------------------------------------------------------------------------------------------- */
void* bfh_bpr_create(void);                                        /* CuBPR::CuBPR      bpr.cu:181 */
void bfh_bpr_destroy(void* h);                                     /* CuBPR::~CuBPR     bpr.cu:222 */
int bfh_bpr_init(void* h, const char* opt_json_path);              /* CuBPR::init       bpr.cu:245 */
int bfh_bpr_get_vdim(void* h);                                     /* CuBPR::get_vdim   bpr.cu:346 */
/* CuBPR::initialize_model bpr.cu:286-308: set_gpu==0 only records the host pointers. */
int bfh_bpr_initialize_model(void* h, float* P, int P_rows, float* Q, float* Qb, int Q_rows,
                             int64_t num_nnz, int set_gpu);
/* CuBPR::set_placeholder bpr.cu:310-320: full rowwise indptr + max chunk nnz. */
int bfh_bpr_set_placeholder(void* h, const int64_t* indptr, size_t batch_size);
/* CuBPR::set_cumulative_table bpr.cu:322-327: int64 cumulative item counts [Q_rows]. */
int bfh_bpr_set_cumulative_table(void* h, const int64_t* table);
/* CuBPR::partial_update bpr.cu:350-430 (CyBPR.add_jobs).  keys == NULL means "use the CSR made
 * resident by bfh_bpr_set_resident_csr". Outputs: sum of log(1+e^-x) when
 * compute_loss_on_training, and the number of (u,pos,neg) samples. */
int bfh_bpr_partial_update(void* h, int start_x, int next_x, const int64_t* indptr,
                           const int32_t* keys, double* loss_sum, double* n_samples);
/* SGDAlgorithm::update_parameters lib/algo.cc:382-465 on the device (no-op for optimizer "sgd"). */
int bfh_bpr_update_parameters(void* h);
/* CuBPR::synchronize bpr.cu:330-344: device_to_host != 0 copies P,Q,Qb into the host arrays. */
int bfh_bpr_synchronize(void* h, int device_to_host);
/* CBPRMF::compute_loss bpr.cc:227-244 (same contract as CuBPR::compute_loss bpr.cu:432). */
int bfh_bpr_compute_loss(void* h, int n, const int32_t* users, const int32_t* positives,
                         const int32_t* negatives, double* loss);

/* ------------------------------------------------------------------------------------------------
 * WARP   (CWARP: include/buffalo/algo_impl/warp/warp.hpp:20-67; same surface as BPR, as
 *         buffalo/algo/warp.py:212-234 expects from an accelerator object)
 * ---------------------------------------------------------------------------------------------- */
void* bfh_warp_create(void);
void bfh_warp_destroy(void* h);
int bfh_warp_init(void* h, const char* opt_json_path);             /* CWARP::init       warp.cc:68 */
int bfh_warp_get_vdim(void* h);
int bfh_warp_initialize_model(void* h, float* P, int P_rows, float* Q, float* Qb, int Q_rows,
                              int64_t num_nnz, int set_gpu);       /* warp.cc:87-94               */
int bfh_warp_set_placeholder(void* h, const int64_t* indptr, size_t batch_size);
int bfh_warp_set_cumulative_table(void* h, const int64_t* table);  /* warp.cc:96-100 (unused)     */
/* CWARP::worker warp.cc:103-173 over one CSR chunk (CyWARP.add_jobs). loss_sum = sum(uj-ui+thr). */
int bfh_warp_partial_update(void* h, int start_x, int next_x, const int64_t* indptr,
                            const int32_t* keys, double* loss_sum, double* n_samples);
int bfh_warp_update_parameters(void* h);                           /* warp.cc:192-201             */
int bfh_warp_synchronize(void* h, int device_to_host);
int bfh_warp_compute_loss(void* h, int n, const int32_t* users, const int32_t* positives,
                          const int32_t* negatives, double* loss); /* warp.cc:205-226             */

/* ------------------------------------------------------------------------------------------------
 * ALS    (CuALS: include/buffalo/cuda/als/als.hpp:20-35)
 * ---------------------------------------------------------------------------------------------- */
void* bfh_als_create(void);                                        /* CuALS::CuALS      als.cu:124 */
void bfh_als_destroy(void* h);
int bfh_als_init(void* h, const char* opt_json_path);              /* CuALS::init       als.cu:230 */
int bfh_als_get_vdim(void* h);                                     /* als.cu:342                   */
int bfh_als_initialize_model(void* h, float* P, int P_rows, float* Q, int Q_rows); /* als.cu:271 */
int bfh_als_set_placeholder(void* h, const int64_t* lindptr, const int64_t* rindptr,
                            size_t batch_size);                    /* als.cu:292                   */
int bfh_als_precompute(void* h, int axis);                         /* als.cu:310 / als.cc:86       */
/* CuALS::partial_update als.cu:346-406 with CALS numerics (als.cc:95-358).  Updated rows
 * [start_x,next_x) are copied back into the host factor array before returning (als.cu:403).
 * keys/vals == NULL: use the CSR made resident by bfh_als_set_resident_csr(axis). */
int bfh_als_partial_update(void* h, int start_x, int next_x, const int64_t* indptr,
                           const int32_t* keys, const float* vals, int axis, double* loss_nume,
                           double* loss_deno);

/* ------------------------------------------------------------------------------------------------
 * Extensions (not in the reference): residency, determinism hooks, measurement, multi-GPU plumbing
 * ---------------------------------------------------------------------------------------------- */
/* Select the GPU for a handle; call before *_init.  Default: current HIP device at *_create. */
int bfh_bpr_set_device(void* h, int device);
int bfh_warp_set_device(void* h, int device);
int bfh_als_set_device(void* h, int device);

/* Keep the whole CSR in HBM (288 GB) instead of re-sending keys every epoch (bpr.cu:362,
 * als.cu:361-364).  indptr: int64[rows] end offsets; keys/vals: [nnz]. */
int bfh_bpr_set_resident_csr(void* h, const int64_t* indptr, const int32_t* keys, int64_t nnz);
int bfh_warp_set_resident_csr(void* h, const int64_t* indptr, const int32_t* keys, int64_t nnz);
int bfh_als_set_resident_csr(void* h, int axis, const int64_t* indptr, const int32_t* keys,
                             const float* vals, int64_t nnz);
/* With resident CSR the per-call write-back of updated rows (als.cu:403) can be deferred. */
int bfh_als_synchronize(void* h, int device_to_host);
/* Fold-in: factor rows for n_rows histories that are not in the model (new users, changed histories; axis 1: new items from their user lists).
 * Not in the reference.  Needs bfh_als_initialize_model only (no placeholder, no resident CSR).
 * CSR as everywhere here: int64 indptr[n_rows] END offsets (no leading 0), int32 keys[nnz], float vals[nnz].  axis 0 solves against Q (keys index
 * items, reg_u), axis 1 against P (keys index users, reg_i); with FF = the Gramian of that factor, per row b of n_b entries (k_j, v_j):
 *     A = FF + alpha sum_j v_j y_kj y_kj^T + reg ada I  (ada = n_b under adaptive_reg, else 1),   y = sum_j (1 + alpha v_j) y_kj,   out[b] = A^-1 y
 * by an exact solve (Cholesky) whatever `optimizer` the handle was initialised with.  n_b == 0 gives the zero row; duplicate keys add up; columns
 * d .. vdim of every row are 0.  Nothing of the model is written, and no state of a training epoch in flight (Gramian, work lists, scratch, the plan
 * read back as "als_last_*") is touched: the call keeps a Gramian per axis of its own, recomputed only when that factor has changed.
 * out: host [n_rows, vdim], or NULL = leave the rows in the device buffer "fold" (bfh_als_device_buffer),
 * valid until the next fold_in / initialize_model / destroy.  Returns after the handle's stream has drained.
 * BFH_ERR_INVALID with a message, before anything is uploaded or launched: a call before initialize_model, axis outside {0, 1}, n_rows < 0, a
 * decreasing indptr, indptr[n_rows - 1] != nnz, NULL arrays with nnz > 0, any key outside [0, rows of the other factor) -- found by a HOST scan
 * of all nnz keys (serving input is not trusted; an out-of-range key never reaches a gather).  BFH_ERR_UNSUPPORTED above vdim 128 (d <= 128 is the
 * limit: there is no dense solve above it).  n_rows == 0 returns 0 and launches nothing.
 * The batch is walked in sub-batches whose scratch slots (vdim^2 + 2 vdim floats per row, 66 KB at vdim 128, one more per row above 4,096
 * entries) stay under 512 MiB -- or one row's, if larger; a row's result does not depend on where the cuts fall.  Rows up to 4,096 entries are
 * bit-reproducible whatever else is in the batch; longer rows sum their chunks with fp32 atomics.
 * bfh_stats: kernel_ms = row pass + solve, optimizer_ms = the solve kernel alone, aux_ms = the Gramian, h2d_bytes / d2h_bytes as the other calls. */
int bfh_als_fold_in(void* h, int axis, int n_rows, const int64_t* indptr, const int32_t* keys,
                    const float* vals, int64_t nnz, float* out);

/* Named integer knobs.  Unknown names fail with BFH_ERR_INVALID.  The "xcd_*" and "im_*" knobs -- everything marked (2) or (3) below, the
 * policies of "hogwild_atomic" -- are BPRMF's: bfh_warp_set_mode does not know them.
 *   "sequential"      1 = one wave walks the chunk in CSR order: the deterministic parity mode.
 *   "hogwild_atomic"  how the SGD (Hogwild) kernels keep the shared factor rows coherent across the 8 XCDs:
 *                       3  BPRMF sgd default: item-major walk (csrc/bpr_item_major.hpp) -- users owned by XCDs (plain
 *                          stores through the owner's L2), the positive item row in registers with bounded-staleness
 *                          atomic flushes, negatives in per-XCD replicas merged by the delta rule;
 *                       1  fp32 atomic adds on the shared item rows, user-major walk (WARP; BPRMF adam/adagrad
 *                          accumulation always uses this);
 *                       2  BPRMF: user-major walk on per-XCD replicas of the item factors, popular rows on atomics;
 *                       0  racy device-coherent write-through stores (CPU Hogwild literally; loses colliding updates).
 *   "xcd_sync_updates" updates between two merges of the per-XCD replicas (default 2^23 for 3, 2^21 for 2);
 *   "xcd_merge_mean"   1 = average instead of sum the replicas' deltas;  "xcd_hot_tau" (permille) tolerated collision
 *                      probability of a plainly stored row, above it the row is updated with atomics;
 *   "xcd_stiff_b", "xcd_stiff_q", "xcd_stiff_p"  (3, permille) curvature assumed by the merge's per-row saturation weights for the item
 *                      biases (default 250 = the logistic loss's 1/4, the multi-GPU exchange's constant), the item factor rows and the
 *                      replicated user rows (default 0 = plain sum): a row whose replicas each took m steps between two merges is merged
 *                      with w = (1 - exp(-n x)) / (n (1 - exp(-x))), x = lr k (m - 1/n) (sum for cold rows -- exactly, up to one step per row -- mean for
 *                      saturated ones);  "xcd_stiff_lr_ref" (3, units of 1e-6, default 1000 = lr 0.001): the learning rate the curvatures were
 *                      calibrated at -- above it they shrink like lr_ref / lr (at a high lr a row sits in the flat part of the sigmoid for most of
 *                      its steps; the constant at every lr, 0, left the biases 19 % low on the reference benchmark's lr 0.05 -> 0.0001 schedule);
 *   "im_user_lr_max"   (3, permille, default 10) learning rate up to which "im_user_replicas" / "im_user_hybrid" apply;
 *   "im_max_stale"     (3) updates of one item row in flight unseen by the other waves, stated at lr 0.05 (scales 1/lr; default 16);
 *   "im_p_nt", "im_neg_limit"  (3) study knobs (non-temporal hint on the P rows; uniform negatives folded into the first rows
 *                      of Q): DESIGN.md 4.1 "what bounds it" -- not for training;
 *   "im_dual"          (3) two triples per wave at vdim <= 128 (the half-waves walk two slices side by side): -1 (default) = for calls
 *                      with 1024 users per queue or more (6144 until round 6), 1 = always, 0 = never;
 *   "im_user_replicas" (3) 1 = per-XCD replicas of P (entries spread over the queues by position, delta rule at the merges)
 *                      instead of one owner XCD per user; -1 (default) = when a call has fewer than 3072 users per queue
 *                      (the shards of an 8-GPU ML-20M run) and lr <= 0.01, 0 = never;
 *   "im_user_hybrid"   (3) otherwise (whole matrices, lr <= 0.01): replicas for the HEAVY users only -- the ones "xcd_hot_tau" would put
 *                      on atomics; 2 (default) = their entries over as few neighbouring queues as needed, 1 = over all, 0 = off;
 *   "im_drift_budget"  (3, permille) lr-weighted positive steps of a row per merge interval above which its negative
 *                      updates also go to the chip-wide copy;  "im_blocks" runs an item's entries are cut into per queue (0 = ceil(160 lr));
 *   "im_presample"     (3) the call's negatives are settled in CSR order before the walk: 2 (default) = the walk computes the first draw
 *                      itself and reads, in its own order, only the rejected ones (uniform sampling on a chunk kept in HBM; else 1),
 *                      1 = every negative at its nnz position, 0 = drawn inside the walk;  "xcd_fresh" re-read a row right
 *                      before storing it (prefetching variants);  "im_drain_only", "im_single_wave", "im_force_queues" test hooks;
 *   "prefetch"         software prefetch of the per-triple rows (user-major: 0/1, default 1; item-major: default 0 = rows
 *                      are read where they are used, 1 = two triples ahead);
 *   "waves_per_cu", "chunk" (nnz positions per wave work item), "als_writeback" (0 = defer), "timing" (1 = record HIP
 *   events around every launch), "epoch";
 *   "als_split_f16"    (ALS, in-place iALS++ rows, d >= 64; default 1) the row Gramian through v_mfma_f32_32x32x16_f16 with every
 *                      operand cut into two round-to-nearest f16 pieces (fp32 accuracy, 5x fewer matrix-core cycles);
 *                      0 = v_mfma_f32_32x32x2_f32;  "als_split_wcut": rows holding a weight alpha*v above this (default 32768) or a
 *                      negative one go through the fp32 instruction + the dense-solve kernel (a scan of the weights, cached per
 *                      chunk, finds them);  "als_pc" (default 1) producer / consumer wave pairs for those rows where they win (d = 96, 128;
 *                      csrc/als_pc.hpp), 2 = also at d = 64, 0 = round 3's wave-per-row kernel everywhere;  "als_inreg" 0 = every row through the scratch slot + als_solve_kernel;
 *                      "als_wide_split" (default 1): 128 < vdim <= 224 on the split-f16 form of als_wide_kernel (from vdim 192 up with the fourth product l l),
 *                      0 = the fp32 instruction (vdim 256 always).
 *                      Which kernel family the last bfh_als_partial_update ran is read back the same way (dptr NULL, the value in *bytes): "als_last_path" 0 none (no rows),
 *                      1 producer / consumer pairs, 2 wave per row solved in registers, 3 scratch slot + als_solve_kernel, 4 als_wide_kernel, 5 als_ialspp_kernel;
 *                      "als_last_split" 1 = split-f16 Gramian;  "als_last_n_work" / "als_last_n_heavy": work items / rows above 4,096 entries of the call's work list;
 *                      "als_last_n_def" / "als_last_n_def_rows": items / whole rows the weight scan sent to the fp32 instruction (0 where the plan did not scan).
 *   "als_fold_solve"   (ALS, bfh_als_fold_in; default 1) the solve of the folded-in rows by als_fold_solve_kernel, a Cholesky all four waves of the
 *                      block take part in; 0 = als_solve_kernel with the llt solver (one wave factors), on the same slots -- kept so that the two can
 *                      be timed alternately in one handle (scripts/fold_in_probe.py);  "als_fold_slot_bytes": the bound on one sub-batch's slot
 *                      scratch (default 512 MiB; tests lower it to move the cuts). */
int bfh_bpr_set_mode(void* h, const char* name, int64_t value);
int bfh_warp_set_mode(void* h, const char* name, int64_t value);
int bfh_als_set_mode(void* h, const char* name, int64_t value);

/* Multi-GPU sharding (one process per GPU, users sharded above this ABI): global position of the
 * shard's first nnz (keeps the counter-based sampler identical to the 1-GPU run) and the number of
 * shards that advance the lr schedule together. */
/* Host-only (no GPU needed): the slice schedule of the item-major sgd walk for `num_queues` (<= 8) queues holding
 * queue_entries[x] interactions each.  slice_len = triples per wave work item (the largest multiple of
 * num_negative_samples <= 64), segments = merge intervals of the call; ticket t of queue x works on slice
 * (t * queue_stride[x]) mod queue_slices[x], segment s takes the tickets [slices*s/segments, slices*(s+1)/segments).
 * What CBPRMF's job queue (algo.hpp:28-69) is to the CPU path; exported so that the schedule can be checked on its own. */
int bfh_bpr_item_major_plan(int num_queues, const int64_t* queue_entries, int num_negative_samples, int64_t sync_updates, int* slice_len,
                            int64_t* segments, int64_t* queue_slices, int64_t* queue_stride);
/* Host-only: the number of consecutive incidences of an item-sorted list that one wave of the gradient gather owns
 * (adam / adagrad BPRMF and WARP).  A run of one item's incidences that crosses a multiple of it is added to its
 * gradient row in two or more parts; exported so that tests can place runs around that bound. */
int bfh_sgd_gather_chunk(void);
int bfh_bpr_set_shard(void* h, int64_t nnz_offset, int num_shards);
int bfh_warp_set_shard(void* h, int64_t nnz_offset, int num_shards);

/* Test hook: apply explicit (u,pos,neg) triples with learning rate lr (sgd) or accumulate their
 * gradients (adam/adagrad), bypassing the sampler. */
int bfh_bpr_update_triples(void* h, int64_t n, const int32_t* users, const int32_t* positives,
                           const int32_t* negatives, double lr);

/* Device pointers for collectives (RCCL through torch.distributed) and zero-copy inspection.
 * BPR/WARP names: "P" "Q" "Qb" "gradP" "gradQ" "gradQb" "countP" "countQ" "velP" "velQ" "velQb" "momP" "momQ" "momQb";
 * ALS names: "P" "Q" "FF", and "fold": the [n_rows, vdim] rows of the last bfh_als_fold_in (NULL / 0 bytes after a call without rows),
 * valid until the next fold_in as well.  *dptr is valid until the next initialize_model / destroy. */
int bfh_bpr_device_buffer(void* h, const char* name, void** dptr, size_t* bytes);
int bfh_warp_device_buffer(void* h, const char* name, void** dptr, size_t* bytes);
int bfh_als_device_buffer(void* h, const char* name, void** dptr, size_t* bytes);
/* hipStream_t the handle launches on (for event timing / stream ordering by the caller). */
void* bfh_bpr_stream(void* h);
void* bfh_warp_stream(void* h);
void* bfh_als_stream(void* h);

/* ---- Multi-GPU inside the library (SURVEY.md section 8(b) "_set_devices" / 8(e)): one process per GPU, one RCCL rank per
 * process.  The reference has no multi-device code; a binding drives it like this:
 *   rank 0:      bfh_comm_unique_id(id, 128)  -> hand the 128 bytes to every rank (MPI / a file / torch's store)
 *   every rank:  comm = bfh_comm_create(world, rank, id, device);  bfh_{bpr,warp,als}_set_comm(h, comm)
 * and from then on the handle exchanges by itself over RCCL / xGMI:
 *   BPRMF sgd  -- users (P rows + their CSR rows) sharded, Q / Qb replicated: at every exchange point ONE ncclAllReduce of
 *                 Q | Qb sums what the ranks changed since the state Z they agree on, and every rank advances
 *                 Z <- Z + w R with a per-row weight w between 1 (cold rows: the deltas are independent steps, SUM) and
 *                 1/world (rows every rank drove to its local equilibrium: MEAN) -- see exchange_weight_kernel.  Default: one
 *                 exchange per partial_update, finished before it returns.  "comm_segments" = k > 1 cuts a call into k
 *                 segments whose exchanges travel on the communicator's stream behind the next segment's walk, the last one
 *                 staying in flight until the next exchange point ("comm_overlap" = 0: until the call returns);
 *                 bfh_*_comm_flush / synchronize / compute_loss finish what is in flight;
 *   adam / adagrad / WARP -- update_parameters sums gradQ | gradQb (| counts) over the ranks before the (then identical)
 *                 optimizer step: exactly the single-GPU result up to summation order (lib/algo.cc:382);
 *   ALS        -- rows of the side being solved sharded, both factor matrices replicated: after partial_update on its
 *                 rows a rank calls bfh_als_publish_rows(h, axis, bounds, world + 1), the uneven all-gather of the solved
 *                 row blocks (a group of ncclBroadcast); FF is recomputed per rank from the identical replica.
 * The communicator is not owned by the handle: destroy the handles first.  bfh_comm_all_reduce_f64 sums host doubles
 * (loss sums) over the ranks. */
int bfh_comm_unique_id(char* out, size_t bytes);
void* bfh_comm_create(int n_ranks, int rank, const char* unique_id, int device);
void bfh_comm_destroy(void* comm);
int bfh_comm_rank(void* comm);
int bfh_comm_size(void* comm);        /* ranks of the LIVE communicator: ncclCommCount, not the number bfh_comm_create was asked for */
int bfh_comm_transport(void* comm, char* out, size_t bytes);   /* "rccl <major.minor.patch>" (libbuffalo_hip_test.so over shared memory: "shm-test") */
int bfh_comm_self_test(void* comm);
int bfh_comm_all_reduce_f64(void* comm, double* values, int n);
int bfh_bpr_set_comm(void* h, void* comm);
int bfh_warp_set_comm(void* h, void* comm);
int bfh_als_set_comm(void* h, void* comm);
int bfh_bpr_comm_flush(void* h);
int bfh_warp_comm_flush(void* h);
int bfh_als_publish_rows(void* h, int axis, const int* bounds, int n_bounds);

int bfh_bpr_get_stats(void* h, bfh_stats* out);
int bfh_warp_get_stats(void* h, bfh_stats* out);
int bfh_als_get_stats(void* h, bfh_stats* out);
int bfh_bpr_reset_stats(void* h);
int bfh_warp_reset_stats(void* h);
int bfh_als_reset_stats(void* h);

/* ------------------------------------------------------------------------------------------------
 * Top-k selection over factor products   (buffalo/parallel/_core.hpp)
 * The consumer of P, Q right after training: ParALS/ParBPRMF.topk_recommendation, most_similar
 * (parallel/base.py:21-28, 46-60) and the validation ranking loop (evaluate/base.py:31-42, 80-82).
 * ---------------------------------------------------------------------------------------------- */
void* bfh_topk_create(void);
void bfh_topk_destroy(void* h);
int bfh_topk_set_device(void* h, int device);
/* parallel::dot_topn _core.hpp:89-142 (Cython dot_topn _core.pyx:39-56; the num_threads argument has no
 * meaning here).  Host arrays in, host arrays out: out_keys/out_scores are [num_queries, k], C order.
 * Candidates j == indexes[i] are skipped when P == Q (same pointer), a non-empty pool restricts the
 * candidates, qb_rows == 0 means "no bias".  Admission rule, tie order and padding follow the
 * reference: only scores > FLT_MIN are ever admitted, kept set = first k by (score desc, index asc),
 * listed by (score desc, index desc); unfilled slots below min(k, q_rows[, pool_size]) read
 * (-1, FLT_MIN), the slots above it (-1, 0.0).  k <= 16384. */
int bfh_topk_dot_topn(void* h, const int32_t* indexes, int num_queries, const float* P, int p_rows, int p_cols,
                      const float* Q, int q_rows, int q_cols, const float* Qb, int qb_rows, int32_t* out_keys,
                      float* out_scores, const int32_t* pool, int pool_size, int k);
/* Same selection with the factor matrices already in HBM (e.g. the "P"/"Q"/"Qb" buffers a training
 * handle returns from bfh_*_device_buffer): no PCIe traffic except indexes/pool in and results out.
 * dP/dQ are device pointers to row-major [rows, ld] floats with ld % 8 == 0 and columns >= d zero
 * (the training layout: ld = vdim); `same` != 0 applies the P == Q self-exclusion. */
int bfh_topk_dot_topn_device(void* h, const int32_t* indexes, int num_queries, const float* dP, int p_rows, const float* dQ,
                             int q_rows, int d, int ld, const float* dQb, int qb_rows, int same, int32_t* out_keys,
                             float* out_scores, const int32_t* pool, int pool_size, int k);
/* "The k best items this user has not seen": bfh_topk_dot_topn with a per-row exclusion, in one sweep.
 * bfh_topk_set_seen binds the training matrix whose rows are never recommended: END-offset CSR (seen_indptr[u] = end of row u, no
 * leading 0), keys ascending per row (repeats allowed), validated as bfh_eval_set_data validates it and kept in HBM on the handle
 * until replaced.
 * bfh_topk_recommend_unseen: row b of out_keys / out_scores is, bit for bit, the row bfh_topk_dot_topn gives for the single query
 * users[b] with `pool` = the items that are not in that user's seen row -- intersected with the call's pool where pool_size > 0 -- under
 * the handle's "flt_min_rule", with the same tie rule and the same padding: with n_b the columns of that per-user pool, the unfilled
 * slots below min(k, q_rows, pool_size, n_b) read (-1, FLT_MIN), the slots above it (-1, 0.0).  A user with nothing left to recommend
 * (n_b == 0) gets (-1, 0.0) in every slot.  There is no self-exclusion (P and Q are different matrices).  Users may repeat and come in
 * any order.  Requires p_rows == num_users and q_rows == num_items of bfh_topk_set_seen; calling it before bfh_topk_set_seen, a user
 * outside [0, num_users) and k outside [1, 16384] are refused with a message.  The "fused" rule of bfh_topk_set_mode picks the path as
 * for bfh_topk_dot_topn (d > 128: dense); the seen items are excluded inside the selection kernels on either path, so exactly k slots
 * per user are selected -- never k + max_seen candidates filtered on the host.
 * bfh_topk_recommend_unseen_device: the same from factor matrices in HBM, arguments as bfh_topk_dot_topn_device without `same`. */
int bfh_topk_set_seen(void* h, int num_users, int num_items, const int64_t* seen_indptr, const int32_t* seen_keys, int64_t nnz);
int bfh_topk_recommend_unseen(void* h, const int32_t* users, int num_queries, const float* P, int p_rows, int p_cols,
                              const float* Q, int q_rows, int q_cols, const float* Qb, int qb_rows, int32_t* out_keys,
                              float* out_scores, const int32_t* pool, int pool_size, int k);
int bfh_topk_recommend_unseen_device(void* h, const int32_t* users, int num_queries, const float* dP, int p_rows, const float* dQ,
                                     int q_rows, int d, int ld, const float* dQb, int qb_rows, int32_t* out_keys,
                                     float* out_scores, const int32_t* pool, int pool_size, int k);
/* "The k rows most similar to this one": cosine top-k that leaves the factors unnormalised (ParALS / ParBPRMF / ParW2V.most_similar,
 * parallel/base.py:21-28, 76-99, 151-169, without the algo.normalize(group) they call first).
 * Fn is what the reference's Algo._normalize (algo/base.py:26-28) makes of F, bit for bit: Fn[j][c] = F[j][c] / sqrt(s_j + float32(1e-8))
 * in float32, s_j = the float32 sum of the float32-rounded squares of row j's columns in numpy's pairwise order (csrc/topk_kernels.hpp:
 * topk_normalize_kernel), square root and division correctly rounded.  Rows that hold NaN or Inf get whatever that arithmetic gives.
 * bfh_topk_normalize: host F [rows, cols] in, host out [rows, cols] = Fn.
 * bfh_topk_normalize_device: the same in HBM, dF and dOut [rows, ld] with ld % 8 == 0; columns [d, ld) of dOut are written as zero, those
 * of dF are not read.  dOut == dF is allowed (what algo.normalize() of a resident model needs).
 * bfh_topk_most_similar: row b of out_keys / out_scores is, bit for bit, the row bfh_topk_dot_topn gives for indexes[b] with P = Q = Fn
 * (the same pointer: a query's own row is excluded), no bias, under the handle's modes (bfh_topk_set_mode), with the same tie rule and the
 * same padding.  F is not written: Fn lives in a buffer of the handle (rows * ld * 4 bytes, ld = cols rounded up to 8) that only grows
 * and is reused across calls.  An index or a pool id outside [0, rows), k outside [1, 16384] and rows or cols below 1 (or cols above
 * 2^24) are refused with a message before anything is launched.  The normalisation counts into aux_ms of bfh_topk_get_stats.
 * bfh_topk_most_similar_device: the same from a factor matrix in HBM, dF [rows, ld] as in bfh_topk_dot_topn_device; dF is not written.
 * bfh_topk_most_similar_vectors: the queries are the vectors V [num_queries, cols] themselves (the np.ndarray key of
 * Algo._get_most_similar_item, algo/base.py:108-119), scored as given against Fn with no self-exclusion: row b is the bfh_topk_dot_topn
 * row of query b with P = V, Q = Fn. */
int bfh_topk_normalize(void* h, const float* F, int rows, int cols, float* out);
int bfh_topk_normalize_device(void* h, const float* dF, int rows, int d, int ld, float* dOut);
int bfh_topk_most_similar(void* h, const int32_t* indexes, int num_queries, const float* F, int rows, int cols,
                          int32_t* out_keys, float* out_scores, const int32_t* pool, int pool_size, int k);
int bfh_topk_most_similar_device(void* h, const int32_t* indexes, int num_queries, const float* dF, int rows, int d, int ld,
                                 int32_t* out_keys, float* out_scores, const int32_t* pool, int pool_size, int k);
int bfh_topk_most_similar_vectors(void* h, const float* V, int num_queries, const float* F, int rows, int cols,
                                  int32_t* out_keys, float* out_scores, const int32_t* pool, int pool_size, int k);
/* parallel::quickselect _core.hpp:69-87 (evaluate/base.py:31-42): column indices of the k largest
 * scores of every row of the host matrix scores[rows, cols]; always returned in descending score
 * order (the reference leaves the order unspecified when sorted == 0).  Ties are broken by the
 * higher column index first (std::nth_element leaves that unspecified). */
int bfh_topk_quickselect(void* h, const float* scores, int rows, int cols, int32_t* result, int k, int sorted);
/* "flt_min_rule" (default 1): 0 admits every score in bfh_topk_dot_topn[_device] -- the selection the
 * validation loop gets from numpy scores + quickselect (algo/base.py:40-55 of the reference).
 * "fused" (default -1): -1 = sweeps of 8192 queries x 8192 candidates or more at d <= 128 take the fused path (thresholds
 * from a column sample, filtered score sweep that writes only candidates, wave-per-row selection; results identical to the
 * dense path), 0 = always the dense score buffer + select, 1 = fused whenever d <= 128; "fused_c0" (with "fused" = 1): the
 * exact number of sampled columns (tests); "wave_select" (default 1): 0 = block-per-row selection inside the fused path;
 * "fast_select" (default 1): 0 = the dense select's multi-pass radix path only.
 * "score_func" (default 0 = dot: everything above, bit for bit; any value but 0 and 1 is refused): 1 = L2, ranking by squared distance -- the
 * consumer of a WARP model trained with score_func "l2" (score = -|p - q|^2, no bias: lib/algo_impl/warp/warp.cc:25-28; in the reference
 * WARP._get_topk_recommendation, _get_most_similar_L2 and _get_scores, algo/warp.py:94-150).  Under 1, for bfh_topk_dot_topn[_device],
 * bfh_topk_recommend_unseen[_device] and bfh_topk_most_similar[_device|_vectors]:
 *   The ranking key -- the definition of the list -- of candidate j for query p is key = fl( mfma(p . q_j) + hb_j ), hb_j = -0.5f * s_j,
 *   s_j = the float32 sum of the float32-rounded squares of row j's d columns (never of its ld) in numpy's pairwise order, the sum
 *   bfh_topk_normalize forms.  -|p - q_j|^2 = 2 * key_exact - |p|^2, so per query the order of the keys is the order of the distances,
 *   nearest first.  hb is a per-column bias and travels where Qb travels: the sweep, the thresholds, the selection, the tie rule
 *   ((key desc, index desc); ties at the k-th place by the running-list rule) and the "fused" rule are those of the dot mode, and the
 *   lists are, key for key, the lists of the same call under "score_func" = 0 with "flt_min_rule" = 0 and Qb = hb.
 *   Every score is admissible, whatever "flt_min_rule" says (a distance has no FLT_MIN start).  qb_rows != 0 is refused with a message:
 *   the L2 score has no bias term.
 *   out_scores[b][r] is the SQUARED DISTANCE of the listed key, positive, smallest first (what _get_most_similar_L2 returns): recomputed
 *   for the k winners straight from the two rows, sum_c fl(fl(q_c - p_c)^2) in float32 in numpy's pairwise order, contraction off -- the
 *   bits of ((Q[j] - p) ** 2).sum(-1) on float32 arrays -- not backed out of the key.  Every slot with key -1 reads +inf.  The list
 *   order is the key's: two neighbours of a list may therefore show distances inverted by no more than tau = 4 max_j eps(p, q_j),
 *   eps(p, q) = 2^-24 [(d + 1) |p| |q| + (d + 3) / 2 |q|^2] (the rounding of the key; derivation in tests/l2_cases.py).
 *   bfh_topk_most_similar[_device|_vectors]: no normalisation, the candidates are the rows of F as given (the device form ranks dF where
 *   it lies, so dF's columns >= d must be zero, as bfh_topk_dot_topn_device asks); index queries leave out their own row, as the cosine form does, _vectors has no exclusion.  bfh_topk_normalize[_device]
 *   is unaffected.
 *   hb lives in a buffer of the handle (q_rows floats, grow-only), made once per call; it and the rescoring count into aux_ms.
 * bfh_topk_get_stats: kernel_ms = score kernels, aux_ms = everything else; merges = rows the fused path handed back to the
 * dense path, exchanges = rows whose ties at the k-th place went to the block-level list selection. */
int bfh_topk_set_mode(void* h, const char* name, int64_t value);
int bfh_topk_get_stats(void* h, bfh_stats* out);
int bfh_topk_reset_stats(void* h);

/* ------------------------------------------------------------------------------------------------
 * Validation on the device   (Evaluable: buffalo/evaluate/base.py:44-148 -- the step the train loop runs after every epoch,
 * buffalo/algo/base.py save_best / early stopping)
 * One handle holds the training matrix (the "seen" items) and the held-out `vali` group in HBM; every call then ranks and scores
 * straight from factor matrices, on the host or already on the device.
 * Ranking (base.py:44-128): per user the topk best items that are NOT in the user's training row -- filter_seen_items (:71-78) is
 * part of the selection, so exactly min(topk, num_items) slots are selected, never topk + max_seen.  Every score is admissible (numpy
 * scores + quickselect, algo/base.py:40-55: no FLT_MIN rule); scores are the bits bfh_topk_dot_topn computes, for every d.  Listing
 * order: unseen items by (score descending, index descending), the order bfh_topk_dot_topn documents; ties that straddle the last place are
 * resolved by the running-list rule of bfh_topk_dot_topn (_core.hpp:115-128) over the unseen items: with t the score of the last place, F the
 * first min(topk, num_items) unseen items by index with score >= t and A the items == t inside F, the members of A with the HIGHEST indices fill
 * the places the items > t leave.  Users with fewer unseen items than topk are padded with -1.
 * Metrics: hit / AP / DCG / accuracy / AUC exactly as base.py:92-122 (AUC with its closing term :114, AP and IDCG over
 * min(len(gt), topk) :97,:119), float64 per user, ground truth = the SET of the user's vali columns.  Users whose training row is empty
 * are skipped and not counted (:86-87), and so are users without vali entries in a caller's `rows`.  All sums have a fixed order: the
 * doubles are the same bits run to run and for every "batch".  The per-user values of the ranking metrics are added one after the other
 * in list order, so the four means are the bits the reference's loop (:117-126) gives from the same per-user values; that chain is
 * one dependent float64 add per user (cost: profiles/eval_first_contact.txt).
 * bfh_eval_set_device is for a fresh handle: once set_data or a ranking has allocated on a device, it is refused.
 * bfh_stats of an eval handle: kernel_ms = ranking (scores + selection), optimizer_ms = ranking metrics, aux_ms = set_data's device
 * work and the score metrics, samples = users counted, launches = ranking calls.
 * ---------------------------------------------------------------------------------------------- */
void* bfh_eval_create(void);
void bfh_eval_destroy(void* h);
int bfh_eval_set_device(void* h, int device);
/* Data._prepare_validation_data (buffalo/data/base.py) once per data set: seen_indptr int64[num_users] END offsets (no leading 0) and
 * seen_keys[nnz] of the rowwise training matrix, keys ascending inside a row; vali_row / vali_col / vali_val [n_vali] the held-out
 * triples in file order (pairs listed twice count once in the ranking metrics and twice in rmse / error, as in the reference).
 * Uploaded once; the ground-truth CSR is built on the device.  Ids outside the matrix, descending keys and offsets that do not end at
 * nnz are refused. */
int bfh_eval_set_data(void* h, int num_users, int num_items, const int64_t* seen_indptr, const int32_t* seen_keys, int64_t nnz,
                      const int32_t* vali_row, const int32_t* vali_col, const float* vali_val, int64_t n_vali);
/* users that have vali entries: the rows a NULL `rows` stands for (vali_rows of base.py:52), or a negative bfh_status */
int bfh_eval_num_rows(void* h);
/* Evaluable._evaluate_ranking_metrics base.py:44-128.  Host factors P [p_rows, p_cols], Q [q_rows, q_cols] (C-contiguous, unpadded;
 * p_rows / q_rows = num_users / num_items of set_data), Qb [q_rows] or qb_rows == 0 for "no bias".  rows == NULL: every user with vali
 * entries, ascending (n_rows is ignored); otherwise the caller's subset in the caller's order -- validation.eval_samples (:58-60)
 * draws it in Python.  out[5] = {ndcg, map, accuracy, auc, N}; N == 0 gives five zeros and BFH_OK.  out_keys: NULL or
 * int32[n_rows, topk], the filtered lists.  topk in [1, 16384]. */
int bfh_eval_ranking(void* h, const float* P, int p_rows, int p_cols, const float* Q, int q_rows, int q_cols, const float* Qb, int qb_rows,
                     const int32_t* rows, int n_rows, int topk, double* out, int32_t* out_keys);
/* the same from matrices in HBM -- dP / dQ / dQb, d, ld as in bfh_topk_dot_topn_device (ld % 8 == 0, columns >= d zero): the "P" / "Q" /
 * "Qb" buffers of a training handle, no factor traffic over PCIe */
int bfh_eval_ranking_device(void* h, const float* dP, int p_rows, const float* dQ, int q_rows, int d, int ld, const float* dQb, int qb_rows,
                            const int32_t* rows, int n_rows, int topk, double* out, int32_t* out_keys);
/* Evaluable._evaluate_score_metrics base.py:130-148: out[2] = {rmse, error} over the vali triples, predictions P[row] . Q[col]
 * (+ Qb[col]) as fp32 dots, |err| and err^2 summed in float64.  No vali entries: two zeros. */
int bfh_eval_scores(void* h, const float* P, int p_rows, int p_cols, const float* Q, int q_rows, int q_cols, const float* Qb, int qb_rows,
                    double* out);
int bfh_eval_scores_device(void* h, const float* dP, int p_rows, const float* dQ, int q_rows, int d, int ld, const float* dQb, int qb_rows,
                           double* out);
/* "batch": users per ranking sweep (0 = as many as a 2 GiB score buffer holds; results do not depend on it), "fast_select",
 * "fused", "fused_c0", "wave_select": as bfh_topk_set_mode, for the ranking's engine ("fused" defaults to -1, by size, here
 * too; the lists and the metrics do not depend on it), "timing".
 * "score_func" (default 0 = dot; 1 = L2; anything else is refused), as bfh_topk_set_mode: under 1 bfh_eval_ranking[_device] is the same
 * seen-aware ranking on the L2 key (metrics unchanged), bfh_eval_scores[_device] predicts fl(1.0f - dist), dist = the float32 bits of
 * ((P[row] - Q[col]) ** 2).sum(-1) in numpy's pairwise order (WARP._get_scores, algo/warp.py:147), |err| and err^2 summed as before,
 * and qb_rows != 0 is refused with a message.
 * bfh_eval_get_stats: merges / exchanges as bfh_topk_get_stats reports them, summed over the rankings. */
int bfh_eval_set_mode(void* h, const char* name, int64_t value);
int bfh_eval_get_stats(void* h, bfh_stats* out);
int bfh_eval_reset_stats(void* h);

/* ------------------------------------------------------------------------------------------------
 * COO -> compressed rows on the device   (buffalo/data/fileio.hpp:263-420)
 * The step right before the training path: _sort_and_compressed_binarization, run once per orientation.
 * Records are stable-sorted by (major, minor) -- duplicates are kept, in input order -- and come back as
 * indptr[num_major] (END offsets: records with major id <= k, no leading zero), out_minor[nnz],
 * out_vals[nnz].  Ids are 0-based here (the reference parses 1-based text and subtracts 1, :396,:401).
 * Stateless; failures are reported through bfh_last_error(NULL).  `stats` may be NULL.
 * ---------------------------------------------------------------------------------------------- */
int bfh_coo_to_csr(const int32_t* major, const int32_t* minor, const float* vals, int64_t nnz, int num_major,
                   int num_minor, int64_t* indptr, int32_t* out_minor, float* out_vals, bfh_stats* stats);

/* The working TEXT file of buffalo's data creation parsed on the device (buffalo/data/fileio.hpp:263-330; the file is what
 * buffalo/data/mm.py:175-234 writes: the MatrixMarket body, one "row col val" line per entry, 1-based ids).
 * bfh_parse_triples: the first `total_lines` lines as the reference's sscanf(line, "%d %d %f") reads them (ids stay 1-based) --
 * bit-identical: what the device cannot guarantee to round like strtof is re-parsed on the host with that very call
 * (stats->merges = number of such lines, 0 on ordinary rating files).
 * bfh_text_to_csr: the same followed by _sort_and_compressed_binarization (:328-420) on the device; sort_key 1 = rowwise
 * (major = row), 2 = colwise (major = col); outputs as bfh_coo_to_csr (0-based minors, END offsets). */
int bfh_parse_triples(const char* text, int64_t bytes, int64_t total_lines, int32_t* rows, int32_t* cols, float* vals, bfh_stats* stats);
int bfh_text_to_csr(const char* text, int64_t bytes, int64_t total_lines, int num_major, int num_minor, int sort_key,
                    int64_t* indptr, int32_t* out_minor, float* out_vals, bfh_stats* stats);

/* ------------------------------------------------------------------------------------------------
 * CFR / CoFactor   (CCFR: include/buffalo/algo_impl/cfr/cfr.hpp:19-45, lib/algo_impl/cfr/cfr.cc;
 * SURVEY.md section 8(f) rank 4) -- the three row updates run on the ALS Gramian / dense-solve kernels.
 * Arrays are the reference's CPU layout: C-contiguous float32 [rows, d] (NOT padded), biases [rows, 1];
 * updated rows are written back into them before a call returns.  d <= 128; optimizers llt, ldlt, manual_cg.
 * ---------------------------------------------------------------------------------------------- */
void* bfh_cfr_create(void);                                                   /* CCFR::CCFR           cfr.cc:14  */
void bfh_cfr_destroy(void* h);                                                /* CCFR::~CCFR          cfr.cc:18  */
int bfh_cfr_set_device(void* h, int device);
int bfh_cfr_init(void* h, const char* opt_json_path);                         /* CCFR::init           cfr.cc:29  */
/* CCFR::set_embedding cfr.cc:70-82: obj_type in user | item | context | item_bias | context_bias */
int bfh_cfr_set_embedding(void* h, float* data, int size, const char* obj_type);
int bfh_cfr_precompute(void* h, const char* obj_type);                        /* CCFR::precompute     cfr.cc:85  */
/* CCFR::partial_update_{user,item,context} cfr.cc:92-313: full END-offset indptr + the chunk's keys/vals; *loss
 * receives the value the reference returns (0 unless the option "compute_loss" is set). */
int bfh_cfr_partial_update_user(void* h, int start_x, int next_x, const int64_t* indptr, const int32_t* keys,
                                const float* vals, double* loss);
int bfh_cfr_partial_update_item(void* h, int start_x, int next_x, const int64_t* indptr_u, const int32_t* keys_u,
                                const float* vals_u, const int64_t* indptr_c, const int32_t* keys_c, const float* vals_c,
                                double* loss);
int bfh_cfr_partial_update_context(void* h, int start_x, int next_x, const int64_t* indptr, const int32_t* keys,
                                   const float* vals, double* loss);
int bfh_cfr_get_stats(void* h, bfh_stats* out);
int bfh_cfr_reset_stats(void* h);

/* ------------------------------------------------------------------------------------------------
 * eALS   (CEALS: include/buffalo/algo_impl/eals/eals.hpp:20-84, lib/algo_impl/eals/eals.cc)
 * Element-wise ALS with a prediction cache in both orientations.  Whole-matrix calls: indptr are END offsets
 * of the full matrix, P [P_rows, d] / Q [Q_rows, d] unpadded, C [Q_rows] the item weights c_i.  The structure
 * handed to precompute_cache stays bound; update / estimate_loss take the same arrays again (only vals are read).
 * ---------------------------------------------------------------------------------------------- */
void* bfh_eals_create(void);                                                       /* CEALS::CEALS            eals.cc:6   */
void bfh_eals_destroy(void* h);
int bfh_eals_set_device(void* h, int device);
int bfh_eals_init(void* h, const char* opt_json_path);                             /* CEALS::init             eals.cc:19  */
int bfh_eals_initialize_model(void* h, float* P, float* Q, float* C, int P_rows, int Q_rows);   /* eals.cc:33 */
/* CEALS::precompute_cache eals.cc:49-100: vhat of every observed entry + the index map to the other orientation */
int bfh_eals_precompute_cache(void* h, int nnz, const int64_t* indptr, const int32_t* keys, int axis);
/* CEALS::update eals.cc:102-115 -> 1, or 0 while a cache is missing; the updated side is copied back into P / Q */
int bfh_eals_update(void* h, const int64_t* indptr, const int32_t* keys, const float* vals, int axis);
/* CEALS::estimate_loss eals.cc:117-174 -> (rmse, loss); both 0 while a cache is missing */
int bfh_eals_estimate_loss(void* h, int nnz, const int64_t* indptr, const int32_t* keys, const float* vals, int axis,
                           float* rmse, float* loss);
int bfh_eals_get_stats(void* h, bfh_stats* out);
int bfh_eals_reset_stats(void* h);

/* ------------------------------------------------------------------------------------------------
 * pLSI   (CPLSI: include/buffalo/algo_impl/plsi/plsi.hpp, lib/algo_impl/plsi/plsi.cc; bound by CyPLSI buffalo/algo/_plsi.pyx)
 * One EM epoch is reset -> partial_update per rowwise batch -> normalize -> swap (buffalo/algo/plsi.py:_iterate).  P [P_rows, d] and
 * Q [Q_rows, d] are the caller's unpadded arrays (the reference's CPU layout) and hold the OLD model; the accumulators live on the
 * device.  partial_update runs the P half-step of its rows and keeps the batch in HBM; normalize transposes what the epoch has seen,
 * runs the Q half-step on it and then normalises; swap makes new -> old and copies both matrices back into the caller's arrays.
 * Every sum has a fixed order: an epoch gives the same bits run to run, for every split into batches, batched or resident.
 * The batches of an epoch are consecutive row ranges; reset comes before the first of them (the reference's accumulators are
 * uninitialised memory until reset, plsi.cc:45-46).  With alpha1 = 0 a user without entries is 0 / 0 = NaN, as in the reference.
 * Modes: "keep_init" 1: initialize_model uploads the caller's arrays as they are (warm start); "raw_accumulators" 1: normalize stops
 * after the Q half-step (the sums of plsi.cc:99-100 stay readable as "P_new" / "Q_new"); "resident" 0: drop the resident matrix.
 * bfh_stats of a pLSI handle: samples = entries of the P half-steps, loaded_rows = factor rows gathered (both half-steps),
 * launches = half-step launches, merges = owners long enough to be split over several waves and summed from partial rows,
 * kernel_ms = P half-steps, optimizer_ms = Q half-steps, aux_ms = transposes, exchange_kernel_ms = the normalisation kernels,
 * allreduce_ms = copies of the model back to the caller (swap, synchronize(1)).
 *
 * Fold-in (bfh_plsi_fold_in): topic rows for histories that are NOT in the model, the word side held fixed.  For history b with entries
 * (c_j, v_j) against the handle's current old Q, from p(0) = init[b] (or 1 / d in every column), for t = 1 .. iters:
 *     acc_k = sum_j max(p(t-1)_k Q[c_j, k], 1e-10f) / norm_j * v_j,  norm_j = sum_k max(...);   p(t)_k = (acc_k + a1) / sum_k (acc_k + a1)
 * with a1 = alpha1 / float(d); out[b] = p(iters), loss[b] = -sum_j log(norm_j) v_j of the last step.  A folded row is bit for bit what
 * the training calls give that row after `iters` epochs in which Q is put back after every epoch (same summation order, a function of the
 * row's length alone), so it depends on its own entries, Q, iters, alpha1 and its init row and on nothing else -- not on the batch it
 * came in.  All steps run in one launch with the row in registers.  A history without entries gives a1 / sum_k a1 in every column
 * (NaN for alpha1 = 0, as in training) and loss 0; keys may repeat, each entry is its own term.  The call reads the old Q only and keeps
 * its own buffers: it may be called anywhere in an epoch (between partial_update and normalize as well) without a trace in the training.
 * Refused with BFH_ERR_INVALID before anything is uploaded or launched: a call before initialize_model, n_rows < 0, iters outside
 * [1, 10000], alpha1 negative or not finite, a decreasing indptr, indptr[n_rows - 1] != nnz, null arrays with nnz > 0, and any key outside
 * [0, Q_rows) -- found by a host scan of all keys, so that no untrusted key reaches a gather.
 * bfh_stats: all five timing fields are taken by training, so the time of the fold kernel is returned in *kernel_ms; per call
 * exchanges += 1, launches += 1, accepted += n_rows, loaded_rows += nnz * iters (rows of Q gathered), h2d_bytes / d2h_bytes as elsewhere.
 * ---------------------------------------------------------------------------------------------- */
void* bfh_plsi_create(void);                                                      /* CPLSI::CPLSI          plsi.cc:14 */
void bfh_plsi_destroy(void* h);                                                   /* CPLSI::~CPLSI / release  plsi.cc:17, 34 */
int bfh_plsi_set_device(void* h, int device);
int bfh_plsi_init(void* h, const char* opt_json_path);                            /* CPLSI::init           plsi.cc:22: d, random_seed; num_workers is ignored */
int bfh_plsi_get_vdim(void* h);                                                   /* row stride of the device buffers, ceil(d / 32) * 32 */
/* CPLSI::initialize_model plsi.cc:42-70: binds P, Q and fills them with |N(0, 1/d)|, rows of P and columns of Q summing to 1 (seeded, on the
 * host: the reference's own stream is not defined, its RNG is shared by an OpenMP loop), then uploads them */
int bfh_plsi_initialize_model(void* h, float* P, int P_rows, float* Q, int Q_rows);
/* 0: upload the caller's arrays again (after buffalo/algo/plsi.py:inherit wrote rows into them); 1: copy the old model back */
int bfh_plsi_synchronize(void* h, int device_to_host);
int bfh_plsi_reset(void* h);                                                      /* CPLSI::reset          plsi.cc:38 */
/* CPLSI::partial_update plsi.cc:72-105: full END-offset indptr [P_rows] + the chunk's keys / vals; *loss = -sum log(norm) v of the chunk */
int bfh_plsi_partial_update(void* h, int start_x, int next_x, const int64_t* indptr, const int32_t* keys, const float* vals, float* loss);
/* the whole rowwise matrix stays in HBM with its transpose (built once); then an epoch is reset -> update_resident -> normalize -> swap */
int bfh_plsi_set_resident_csr(void* h, const int64_t* indptr, const int32_t* keys, const float* vals, int64_t nnz);
int bfh_plsi_update_resident(void* h, float* loss);                               /* plsi.cc:72-105 over the resident matrix */
int bfh_plsi_normalize(void* h, float alpha1, float alpha2);                      /* the Q sums of plsi.cc:100, then CPLSI::normalize plsi.cc:107-125 */
int bfh_plsi_swap(void* h);                                                       /* CPLSI::swap           plsi.cc:127 */
/* Fold-in (see above).  CSR as everywhere: indptr = int64 END offsets [n_rows], no leading 0.  init: host [n_rows, d] unpadded or NULL (uniform
 * start); out: host [n_rows, d] unpadded, or NULL to leave the rows in device buffer "fold"; loss: [n_rows] doubles or NULL (the build without
 * the loss); kernel_ms: NULL or the HIP-event time of this call's kernel.  Returns after the stream has drained; n_rows == 0 returns 0 and
 * launches nothing. */
int bfh_plsi_fold_in(void* h, int n_rows, const int64_t* indptr, const int32_t* keys, const float* vals, int64_t nnz, int iters, float alpha1,
                     const float* init, float* out, double* loss, double* kernel_ms);
int bfh_plsi_set_mode(void* h, const char* name, int64_t value);
/* "P", "Q": the old model [rows, vdim] (what bfh_topk_dot_topn_device ranks from); "P_new", "Q_new": the accumulators; "fold": the rows of the
 * last fold_in [n_rows, vdim], columns >= d zero, valid until the next fold_in / initialize_model / destroy */
int bfh_plsi_device_buffer(void* h, const char* name, void** ptr, size_t* bytes);
int bfh_plsi_get_stats(void* h, bfh_stats* out);
int bfh_plsi_reset_stats(void* h);

/* ------------------------------------------------------------------------------------------------
 * Word2Vec, skip-gram with negative sampling   (CW2V: include/buffalo/algo_impl/w2v/w2v.hpp, lib/algo_impl/w2v/w2v.cc; bound by CyW2V
 * buffalo/algo/_w2v.pyx; driven by buffalo/algo/w2v.py: initialize_model, launch_workers, add_jobs per batch and iteration, join)
 * One GPU.  L0 [V, d] is the caller's unpadded array (the reference's layout); on the device L0 and L1 are [V, vdim], vdim = ceil(d/32)*32, pad
 * columns zero; L1 exists on the device only and is zero after initialize_model.  index[index_size] maps a word of the stream to its vocabulary
 * id + 1 (0 = below min_count), scale[V] the subsampling thresholds, dist[V] the cumulative negative-sampling table (w2v.py:91-157).
 * The reference's worker threads and its clock-driven learning rate are replaced by stated functions of the stream:
 *   jobs      cut by the rule of add_jobs (w2v.cc:158-193): non-empty sentences are added while job_size + size <= batch_size, otherwise the job is
 *             queued and a new one starts; batch_size < 0 -> 10000, a missing key -> 0 (one sentence per job);
 *   alpha     of a job = max(min_lr, lr - (lr - min_lr) * processed / (total_word_count * num_iters)) (w2v.cc:344-347), `processed` = words of all
 *             earlier jobs since launch_workers, counted BEFORE subsampling: the reference's schedule when no job waits in the queue;
 *   draws     counter_draw(seed = random_seed, stream, pos, slot, epoch, attempt) -> o0 (csrc/common.hpp: Philox4x32-10,
 *             ctr = (pos lo, pos hi, attempt, epoch << 8 | slot), key = (seed, 0x5bf03635 ^ stream)), where `pos` is the GLOBAL offset of a
 *             word in the stream (the offset the full indptr gives it, so a split into batches changes no draw) and `epoch` =
 *             processed / total_word_count at the start of the add_jobs call (mode "epoch" >= 0 overrides it):
 *               stream 2  subsampling: r1 = o0 at the word's pos (slot 0, attempt 0); the word is dropped when scale[id] <= r1 (w2v.cc:232);
 *               stream 3  window: b = (uint64(o0) * window) >> 32 at the centre's pos (slot 0, attempt 0); centre i of the n kept words of a
 *                         sentence is paired with every j in [max(0, i - window + b), min(n, i + window + 1 - b)), j != i (:239-245);
 *               stream 4  negative k = 0 .. num_negative_samples - 1 of pair (i, j): pos = the centre's, slot = j - i + window,
 *                         attempt = (k << 16) | retry, r3 = (uint64(o0) * dist[V - 1]) >> 32, word = lower_bound(dist, V, r3); retry = 0, 1, ...
 *                         while the word equals the target W[i] (:248-256; given up after 65535 retries);
 *   update    per pair (w2v.cc:274-320): l0 = L0[W[j]] as it is before the pair; for the rows L1[W[i]] (label 1), then the negatives (label 0),
 *             one after the other: f = row . l0; g = label - 1 (f > 6), label (f < -6), else label - table[(int)((f + 6) * 83)] in float32;
 *             g = (float)(g * alpha); work += g * row; row += g * l0; after the last row L0[W[j]] += work.  Products are rounded before they
 *             are added.  Loss terms as :304-309, float64 per work item, the items added in a fixed order.
 * bfh_w2v_init refuses window > 127 (BFH_ERR_INVALID: the slot has 8 bits) and d > 256 (BFH_ERR_UNSUPPORTED); initialize_model refuses a
 * vocabulary of fewer than 2 words when negatives are requested and a dist that is not non-decreasing (BFH_ERR_INVALID).
 * Modes: "sequential" 1 = one wave walks the work items in stream order with the same update code (the parity mode);
 *   "hogwild_atomic" how concurrent lane groups write the shared rows: 1 (default) = global_atomic_add_f32 on contiguous row segments (no update is
 *   lost), 0 = device-coherent read-modify-write stores (the CPU's Hogwild literally; colliding updates are lost) -- either setting gives the same
 *   bits under every schedule without conflicts;  "chunk" centres of one sentence per work item (default 64; 0 = a whole sentence);
 *   "epoch" (-1 = from `processed`);  "timing".
 * bfh_stats of a W2V handle: samples = pairs, scored_negatives = negatives used, accepted = words kept by the subsampling, loaded_rows = redraws
 * of a negative that hit the target, launches / kernel_ms = the update kernel, aux_ms = subsampling and planning.
 * ---------------------------------------------------------------------------------------------- */
void* bfh_w2v_create(void);                                                       /* CW2V::CW2V            w2v.cc:66 */
void bfh_w2v_destroy(void* h);                                                    /* CW2V::~CW2V / release w2v.cc:73, 79 */
int bfh_w2v_set_device(void* h, int device);
/* CW2V::init w2v.cc:85: d, window, num_negative_samples, num_iters, lr, min_lr, random_seed, batch_size, compute_loss_on_training; num_workers is ignored */
int bfh_w2v_init(void* h, const char* opt_json_path);
int bfh_w2v_get_vdim(void* h);                                                    /* row stride of the device buffers */
/* CW2V::initialize_model w2v.cc:104-122; binds L0 (it is read now and rewritten by join / synchronize(1)) and copies index, scale, dist */
int bfh_w2v_initialize_model(void* h, float* L0, int L0_rows, const int32_t* index, int index_size, const uint32_t* scale, const int32_t* dist,
                             int64_t total_word_count);
int bfh_w2v_launch_workers(void* h);                                              /* w2v.cc:132: `processed`, alpha and the loss start over */
/* CW2V::add_jobs w2v.cc:143-194 and the workers' part of it (:197-320), finished on return: full END-offset indptr, the chunk's words.
 * Refused before launch_workers and after join. */
int bfh_w2v_add_jobs(void* h, int start_x, int next_x, const int64_t* indptr, const int32_t* sequences);
/* CW2V::join w2v.cc:364: copies L0 back into the caller's array; *loss = the loss summed since launch_workers (0 unless compute_loss_on_training;
 * the reference returns 0.0) */
int bfh_w2v_join(void* h, double* loss);
int bfh_w2v_synchronize(void* h, int device_to_host);                             /* 0: upload the bound L0 again; 1: copy L0 back */
int bfh_w2v_set_mode(void* h, const char* name, int64_t value);
/* "L0", "L1": float32 [V, vdim].  Of the last add_jobs call, offsets relative to the call's first word: "kept" int32 / "kept_pos" int64 (global
 * positions) / "window_b" int32, one slot per word of the chunk, the kept words of sentence s in order from the sentence's own offset up to
 * "sent_end"[s] (int64, one per sentence of the call). */
int bfh_w2v_device_buffer(void* h, const char* name, void** ptr, size_t* bytes);
void* bfh_w2v_stream(void* h);
int bfh_w2v_get_stats(void* h, bfh_stats* out);
int bfh_w2v_reset_stats(void* h);
/* Host-only: the 1000-cell sigmoid table of CW2V::build_exp_table w2v.cc:124-130 as the update kernel holds it */
int bfh_w2v_exp_table(float* out1000);
/* Test hook: explicit pairs, applied in order by one wave through the update code of add_jobs with learning rate alpha; inputs [n] are the rows of
 * L0, outputs [n, n_out] the rows of L1, the target (label 1) first */
int bfh_w2v_update_pairs(void* h, int64_t n, const int32_t* inputs, const int32_t* outputs, int n_out, double alpha);

/* ------------------------------------------------------------------------------------------------
 * SPPMI matrix of a stream  (CoFactor's context input)
 * Replaces, in HBM and without text files: the pair lines of buffalo/data/stream.py:257-267 (every event with the
 * `windows` events after it in its user's sequence, both orientations), _parallel_build_sppmi
 * (buffalo/data/fileio.hpp:109-254: appearances, pmi = log(cnt) + log(D) - log(app[probe]) - log(app[c]), shift
 * log(k), entries with sppmi > 0, values carried with the six significant digits of the reference's text output;
 * the group of the largest id that has lines is never written by the reference -- it flushes a group when the next id
 * begins and not at end of file, :182-250 -- and is left out here as well) and the sort + compression of its output
 * (stream.py:169-195).
 * bfh_sppmi_build: `indptr` are END offsets [num_users] over the 0-based `items` of the stream; reports the number of
 * entries and D (sppmi_total_lines).  bfh_sppmi_fetch copies the group out: indptr_out[num_items] (END offsets),
 * keys_out[nnz], vals_out[nnz], rows ascending, columns ascending inside a row, a pair (p, p) listed twice as the
 * reference lists it.  (The reference sorts its output by row only, so inside a row it keeps std::unordered_set
 * iteration order; per row the entries here are the same multiset, bit for bit -- tests/test_oracle_ref_fileio.py.)
 * ---------------------------------------------------------------------------------------------- */
void* bfh_sppmi_create(void);
void bfh_sppmi_destroy(void* h);
int bfh_sppmi_build(void* h, const int64_t* indptr, const int32_t* items, int num_users, int num_items, int windows, int k,
                    int64_t* nnz, int64_t* total_lines);
int bfh_sppmi_fetch(void* h, int64_t* indptr_out, int32_t* keys_out, float* vals_out);
int bfh_sppmi_get_stats(void* h, bfh_stats* out);

/* ------------------------------------------------------------------------------------------------
 * Stream database  (the Stream half: text -> events, records, groups, counts)
 * Replaces, in HBM: the per-token Python loops of Stream._create / _create_working_data (buffalo/data/stream.py:81-158,
 * 197-271) and the second walk over all events of W2V.build_vocab (buffalo/algo/w2v.py:91-100).  Every output is an
 * integer array (counts as float where the reference writes them as values) and equals the reference's bit for bit.
 *
 * Lines end at "\n", "\r\n" or a lone "\r" (Python's text mode); a last line without a terminator counts, a text
 * that ends in a terminator adds no line.  White space is the space, \t, \n, \v, \f, \r and \x1c-\x1f (what
 * str.strip() / str.split() remove among the bytes below 0x80).  Bytes >= 0x80 always belong to tokens: white space
 * that exists only in Unicode (U+0085, U+00A0, U+2028, ...) is NOT a separator here.
 *
 * bfh_stream_set_vocabulary (stream.py:120-122): `names` = the bytes of the item-id file; item i (0-based) is line i
 *   stripped.  The names are uploaded and put into an open-addressing table on the device.  Two equal names are
 *   refused (BFH_ERR_INVALID; the reference's dict would shrink and idmap could not be filled); an empty name is
 *   allowed and matches no token.  *num_items = the number of lines.
 * bfh_stream_build (stream.py:216-256): `text` = the bytes of the main file, line u is user u, its tokens (maximal
 *   runs of bytes that are not white space, of any length) are its events.  A token that is no name is the
 *   reference's KeyError: BFH_ERR_INVALID, the message names the 1-based line and the token (cut at 64 bytes) of the
 *   first such token of the file.  vali_n > 0 is the `newest` split (:224-231): the last min(vali_n, max(len - 1, 0))
 *   events of a user are held out, of them the distinct items are kept in order of first appearance.  sample_pos !=
 *   NULL is the `sample` split (:232-245): n_sample ascending global event indices, each < the number of events, drawn
 *   by the caller (base.py:220-226); those events are held out in order.  Both at once, or positions that are not
 *   ascending or out of range: BFH_ERR_INVALID.  Train events = the events not held out, in order.  Records = the
 *   working file of internal_data_type "matrix" (:253-254): users ascending, per user one record per distinct train
 *   item in order of first appearance, val = its count.  Held-out triples = the same over the held list (:255-256).
 *   out_counts = {num_users, num_events, num_train, num_records, num_vali}.  The next build replaces the result; the
 *   vocabulary stays.
 * The fetches are refused before a successful build:
 *   fetch_events   the rowwise group of internal_data_type "stream" (:160-164, order kept): indptr[num_users] END
 *                  offsets, items[num_train] -- the two arrays bfh_sppmi_build and bfh_w2v_add_jobs take;
 *   fetch_records  rows / cols / vals [num_records], 0-based;
 *   fetch_group    the first min(max_records, num_records) records (max_records < 0: all) sorted and compressed on the
 *                  device like bfh_coo_to_csr: sort_key 1 = rowwise (indptr[num_users]), 2 = colwise
 *                  (indptr[num_items]).  The cut is the reference's: its header count is fixed before a `sample`
 *                  split (stream.py:100-120, base.py:224-226) and the sorter keeps the first total_lines records;
 *   fetch_vali     rows / cols / vals [num_vali] in the order met (the value reordering of base.py:241-253 stays
 *                  with the caller);
 *   fetch_counts   counts[num_items]: occurrences of every item among the train events (`uni` of w2v.py:91-100).
 * bfh_stats of a stream handle (summed until reset): samples = tokens, accepted = train events, merges = records,
 *   loaded_rows = table probes beyond a token's first slot, kernel_ms = token boundaries + lookup, aux_ms = the rest
 *   (uploads, table build, splits, sorts, counts), h2d_bytes / d2h_bytes.
 * ---------------------------------------------------------------------------------------------- */
void* bfh_stream_create(void);
void bfh_stream_destroy(void* h);
int bfh_stream_set_device(void* h, int device);
int bfh_stream_set_vocabulary(void* h, const char* names, int64_t bytes, int* num_items);
int bfh_stream_build(void* h, const char* text, int64_t bytes, int vali_n, const int64_t* sample_pos, int64_t n_sample,
                     int64_t out_counts[5]);
int bfh_stream_fetch_events(void* h, int64_t* indptr, int32_t* items);
int bfh_stream_fetch_records(void* h, int32_t* rows, int32_t* cols, float* vals);
int bfh_stream_fetch_group(void* h, int sort_key, int64_t max_records, int64_t* indptr, int32_t* keys, float* vals);
int bfh_stream_fetch_vali(void* h, int32_t* rows, int32_t* cols, float* vals);
int bfh_stream_fetch_counts(void* h, int64_t* counts);
int bfh_stream_get_stats(void* h, bfh_stats* out);
int bfh_stream_reset_stats(void* h);

/* ------------------------------------------------------------------------------------------------
 * MatrixMarket database  (the MatrixMarket half: text file -> rowwise / colwise groups,
 * validation triples, value_prepro)
 * Replaces, in HBM: the header loop (buffalo/data/mm.py:110-165), the `sample` split (data/base.py:210-238,
 * mm.py:167-234), _build_data for both groups (base.py:399-451, fileio.hpp:263-420), fill_validation_data
 * (base.py:240-253) and the three value transforms of buffalo/data/prepro.py.  Every output equals the database the
 * reference's MatrixMarket(opt).create() writes, bit for bit, with ONE stated exception: ImplicitALS (below).
 *
 * bfh_mm_set_value_prepro (base.py:23-27, prepro.py): NULL or "" = none (identity); "OneBased": every value 1.0
 *   (prepro.py:25-27); "MinMaxScalar" (a = min, b = max; prepro.py:33-58): value_min starts at +inf and value_max at
 *   0.0, the one object sees the rowwise train values, then scales the rowwise group, then sees the held-out values
 *   (which come back unscaled), then the colwise values, then scales the colwise group -- so the colwise group is
 *   scaled with a range the held-out values may have widened.  Scaling is ((v - value_min) / (value_max - value_min))
 *   * (b - a) + a with every operation rounded to binary32 (b - a is formed in double and rounded once), or, when
 *   value_max - value_min < 1e-8, every value = (float)b.  "ImplicitALS" (a = epsilon > 0; prepro.py:68-69):
 *   q = v / (float)epsilon and s = 1 + q in binary32, then the CORRECTLY ROUNDED binary32 of log(s) -- the reference's
 *   numpy float32 log is within 1 ulp of that and differs between CPUs, so this library defines the transform by the
 *   rounded value.  Any other name, "SPPMI" included (mm.py:104-106): BFH_ERR_UNSUPPORTED; epsilon <= 0: BFH_ERR_INVALID.
 *   The setting stays until it is changed and applies to the builds after it.
 * bfh_mm_build (mm.py:236-279): `text` = the bytes of the main file as they lie on disk.  Lines end at "\n", "\r\n"
 *   or a lone "\r" (Python's text mode); a last line without a terminator counts.  The header -- the leading lines
 *   whose stripped form starts with "%" (mm.py:154-159), then "num_users num_items num_nnz" -- is read on the host.  A
 *   file on which mm.py:156 (stripped line) and mm.py:250 (raw line) disagree about where the header ends (white space in
 *   front of a "%") is refused.  Only the first num_nnz body lines count (fileio.hpp:312-320); every one is parsed as
 *   sscanf(line, "%d %d %f") parses it (fileio.hpp:300-303; same bit-identity rule as bfh_parse_triples).  The held-out
 *   values are parsed the same way; the reference reads them with Python's float() and narrows to binary32, which can
 *   differ only for a decimal string within 2^-53 (relative) of the midpoint of two neighbouring binary32 values.
 *   `sample_pos` = n_sample STRICTLY ascending body-line indices (0 = the first body line), each < num_nnz - 1 -- the
 *   positions base.py:220-226 draws, sorted (mm.py:187); NULL with n_sample 0 = no split.  Train entries = the body lines
 *   [0, num_nnz) that are not held out, in file order.  Refused with BFH_ERR_INVALID, the message naming the 1-based
 *   file line where there is one: positions not strictly ascending or out of range; fewer than num_nnz body lines (the
 *   reference aborts, fileio.hpp:325); a body line that is not "int int float"; two held-out lines with the same
 *   (row, col) (scipy sums them and base.py:253 cannot assign); an id outside the matrix (as bfh_text_to_csr); a value
 *   that is not finite while MinMaxScalar is set.
 *   out_counts = {num_users, num_items, header_nnz, num_header_lines (the size line included), num_train, num_vali}.
 *   The next build replaces the result.
 * The fetches are refused before a successful build:
 *   fetch_group        sort_key 1 = rowwise (indptr[num_users]), 2 = colwise (indptr[num_items]): the train entries
 *                      sorted and compressed on the device as bfh_coo_to_csr does (END offsets, 0-based keys,
 *                      num_train entries), values transformed (base.py:399-451);
 *   fetch_vali         rows / cols [num_vali] 0-based in file order; vals [num_vali] in (row, col) order (base.py:249-253:
 *                      csr_matrix(...).data) and transformed -- value k does NOT belong to triple k, as in the
 *                      reference's database;
 *   fetch_value_range  {value_min, value_max} used for the rowwise group, {value_min, value_max} used for the colwise
 *                      group (prepro.py:42-45); MinMaxScalar only, else BFH_ERR_INVALID.
 * bfh_mm_set_mode: "vali_file_order" 0 (default) = the reference's value order above; 1 = value k belongs to triple k.
 * bfh_stats of an mm handle (summed until reset): samples = body lines, accepted = train entries, merges = lines handed
 *   to the host parser, kernel_ms = line ends + parse, aux_ms = the rest (upload, split, prepro, sorts), h2d_bytes /
 *   d2h_bytes.
 * ---------------------------------------------------------------------------------------------- */
void* bfh_mm_create(void);
void bfh_mm_destroy(void* h);
int bfh_mm_set_device(void* h, int device);
int bfh_mm_set_value_prepro(void* h, const char* name, double a, double b);
int bfh_mm_set_mode(void* h, const char* name, int64_t value);
int bfh_mm_build(void* h, const char* text, int64_t bytes, const int64_t* sample_pos, int64_t n_sample, int64_t out_counts[6]);
int bfh_mm_fetch_group(void* h, int sort_key, int64_t* indptr, int32_t* keys, float* vals);
int bfh_mm_fetch_vali(void* h, int32_t* rows, int32_t* cols, float* vals);
int bfh_mm_fetch_value_range(void* h, float out[4]);
int bfh_mm_get_stats(void* h, bfh_stats* out);
int bfh_mm_reset_stats(void* h);

#ifdef __cplusplus
}
#endif
#endif /* BUFFALO_HIP_H_ */
