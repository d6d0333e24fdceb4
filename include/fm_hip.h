/*
 * fm_hip.h — C-ABI of the MI355X factorization-machine SGD hot path.
 *
 * This is the drop-in seam for Rainbowboys/fm_spark.  The reference has no FFI of its
 * own: the hot path is the fold body of FactorizationMachinesSGD.runMiniBatchSGD
 * (src/main/scala/org/apache/spark/ml/fm/FactorizationMachinesSGD.scala:116-211) plus the
 * DataFrame plan it builds through FactorizationMachinesModel.calcLossGrad
 * (FactorizationMachinesModel.scala:135-234).  Each entry point below names the reference
 * code it replaces.  A JNI binding for the Scala side is sketched in INTEGRATION.md.
 *
 * Conventions
 *   - plain C types only; every pointer argument is caller-owned and only borrowed for
 *     the duration of the call (host pointers unless the name says _device);
 *   - return codes: FM_OK (0) success, FM_NOTHING_TO_DO (1) an empty mini-batch
 *     (FactorizationMachinesSGD.scala:126-128), negative = error; the message is available
 *     from fm_last_error() on the calling thread.  No C++ exception, abort or exit crosses
 *     this boundary;
 *   - one fm_ctx owns one device's tables, or -- fm_config.parallel != FM_PARALLEL_NONE -- every
 *     rank of a multi-GPU job that this process drives: n_gpus devices from ONE host thread, the
 *     table row-sharded (or replicated) across them, the exchanges done inside the library over
 *     RCCL (xGMI), as SURVEY §8(b) Threading asks of the Spark driver.  Calls on one context are
 *     serialised by an internal mutex; independent contexts may run concurrently
 *     (CrossValidator keeps several models alive at once).
 *   - arithmetic: tables are fp32 on the device, accumulations fp64; inputs/outputs fp64.
 */
#ifndef FM_HIP_H
#define FM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FM_OK 0
#define FM_NOTHING_TO_DO 1
#define FM_ERR_ARG (-1)
#define FM_ERR_OOM (-2)
#define FM_ERR_HIP (-3)
#define FM_ERR_RCCL (-4)
#define FM_ERR_STATE (-5)

#define FM_PARALLEL_NONE 0       /* this context is one table (or one manual shard, shard_index/count) */
#define FM_PARALLEL_SHARDED 1    /* rows sharded by id % R over the job's R ranks, owner-computes */
#define FM_PARALLEL_REPLICATED 2 /* every rank holds the whole table; gradient all-reduce */
#define FM_TRANSPORT_AUTO 0      /* RCCL, unless a device repeats in devices[] (then COPY) */
#define FM_TRANSPORT_RCCL 1      /* RCCL send/recv and all-reduce over xGMI */
#define FM_TRANSPORT_COPY 2      /* one process only: device-to-device copies between the ranks */
#define FM_MAX_LOCAL 16
#define FM_FUSE_DEFAULT 0 /* fm_config.fuse_single: the library's choice (tables above 256 MB) */
#define FM_FUSE_ON 1
#define FM_FUSE_OFF (-1)
#define FM_WIRE_FP32 0 /* fm_config.wire: the owners' partial sums cross as fp32 (default) */
#define FM_WIRE_FP64 1 /* ... as fp64: the sharded step sums every sample in fp64, as the single table */
#define FM_LOSS_SQUARED 0  /* fm_config.loss: the reference's squared error on the label (default) */
#define FM_LOSS_LOGISTIC 1 /* log loss of sigma(yhat) against labels in [0, 1] */
#define FM_LOSS_BPR 2      /* pairwise ranking loss over each positive row and the negatives behind it */

typedef struct fm_ctx fm_ctx;
typedef struct fm_batch fm_batch;
typedef struct fm_lists fm_lists;

/* Model hyper-parameters fixed at creation.
 * num_features : feature ids are int32 in [0, num_features) (README.md:7 "<= Int.MaxValue").
 * k            : dimFactorization (FactorizationMachines.scala:26, >= 1).
 * w0           : globalBias (FactorizationMachinesModel.scala:45); fit always uses 0.0
 *                (FactorizationMachinesSGD.scala:246).
 * init_sd/seed : createInitialModel's N(0, initialSd^2) draw (FactorizationMachinesSGD.scala:234-241),
 *                made deterministic (the reference's draw is unseeded).
 * shard_index/shard_count : (parallel == FM_PARALLEL_NONE) row sharding by feature hash for a
 *                caller that drives the fm_shard_* phases itself; this context owns the ids with
 *                id % shard_count == shard_index (shard_count 1 = whole table).
 * parallel     : FM_PARALLEL_SHARDED / _REPLICATED: this context drives n_gpus local ranks
 *                (devices[0..n_gpus)) of a job of R = n_procs * n_gpus ranks; global rank of local
 *                rank l = proc_rank * n_gpus + l (every process uses the same n_gpus).  Mini-batches
 *                given to it are split by rows, contiguously, over the local ranks; the global
 *                miniBatchSize is the sum over all ranks (SGD.scala:124).  Replaces the shuffles
 *                S1/S2/S5/S6 of SURVEY §2b (Model.scala:155-164, SGD.scala:148-166).
 * transport    : how the ranks exchange (FM_TRANSPORT_*).  n_procs > 1 needs RCCL and comm_id:
 *                process 0 calls fm_comm_unique_id and hands the 128 bytes to the others by any
 *                channel (Spark broadcast, torch.distributed, a file).
 *                RCCL with R > 1 ranks has not run on hardware yet (every test box had one
 *                MI355X): the R > 1 protocol is verified through the COPY transport only.
 * fuse_single  : FM_FUSE_ON: a batch prepared by fm_batch_prepare on a single-table context with
 *                k <= 16 takes the fused step -- the forward updates every row whose feature has one
 *                entry in the batch, the segmented update only the rest (the same table as the
 *                unfused step within fp64 summation order); FM_FUSE_DEFAULT (0): the same, for tables
 *                larger than the 256-MB Infinity Cache; FM_FUSE_OFF: never.  Multi-GPU contexts
 *                never fuse (a sharded owner's fused step measured slower than the unfused one at
 *                R = 8 and at world 1).
 * xchg_chunks  : sharded step with R > 1: the owners' partial pass runs in this many chunks, each
 *                sent while the next is computed (0 = the default, 4; 1 = one pass then one
 *                all-to-all; at most 64).  Every process of a job must pass the same value.
 * wire         : sharded step and predict: the number format in which the owners' partial forward sums
 *                travel to the requesters (owner -> requester; see the fm_shard_* block).
 *                FM_WIRE_FP32 (0, default): each owner rounds its share of a sample's sums to fp32.
 *                FM_WIRE_FP64: the shares stay fp64, so a sample's S, sum v^2 x^2 and sum w x are
 *                fp64 sums over all of its entries, rounded once -- what the single table computes
 *                (the reference sums in Double, FactorizationMachinesSGD.scala:145-154); the partial
 *                direction carries twice the bytes.  The S rows going back are fp32 either way.  Every
 *                process of a job must pass the same value.  Any other value is FM_ERR_ARG, and so is
 *                FM_WIRE_FP64 with FM_PARALLEL_REPLICATED (the replicated gradient all-reduce is fp32;
 *                the flag would change nothing there).  A context that exchanges nothing accepts it
 *                and its step and predict never read it (FM_PARALLEL_NONE with shard_count 1); a
 *                caller that drives the fm_shard_* phases itself (FM_PARALLEL_NONE, shard_index /
 *                shard_count) gets the format of that context's own value.
 * loss         : the training objective of fm_step / fm_step_batch, a property of the context.
 *                FM_LOSS_SQUARED (0, default): the reference's step, sum (yhat - y)^2 with its own
 *                g_w = x*yhat - y, unchanged in every bit.
 *                FM_LOSS_LOGISTIC: pointwise, labels y in [0, 1] (NOT checked on the device: a label
 *                outside gives the gradient of that formula, not an error; check them where they are
 *                host data).  r_s = sigma(yhat_s) - y_s; a row with at least one entry adds
 *                softplus(yhat_s) - y_s*yhat_s to loss_sum and 1 to n_loss_rows.
 *                FM_LOSS_BPR: pairwise, over groups of g = fm_batch_group(batch) consecutive rows: row
 *                p = q*g is the positive, rows p+1 .. p+g-1 its negatives (fm_batch_sample_pairs' layout).
 *                With d_j = yhat_p - yhat_{p+j}: r_{p+j} = sigma(-d_j), r_p = -sum_j sigma(-d_j); the group
 *                adds sum_j softplus(-d_j) to loss_sum and one loss row per (positive, negative) pair.  A
 *                row without entries scores w0 and takes part.  Labels are not read.
 *                Both: w -= eta/m * sum_s x*r_s and V -= eta/m * sum_s r_s*(x*S - v*x^2), the true gradient
 *                (m = n_rows, also under BPR), then the soft threshold as ever.  r is formed in fp64 from
 *                the score as the step stores it -- yhat rounded to fp32 -- in forms that stay finite for
 *                every finite score, and rounded to fp32 once.  A stage of its own between the forward
 *                and the update (profile name "objective"); a squared context launches nothing new.
 *                A non-squared loss needs parallel == FM_PARALLEL_NONE and shard_count == 1 (FM_ERR_ARG
 *                naming the loss: multi-GPU objectives are left for later), refuses fuse_single ==
 *                FM_FUSE_ON (the fused forward applies singleton rows with the squared residual before
 *                the stage runs) and never fuses under FM_FUSE_DEFAULT (fm_fuse_active is 0).  fm_repl_grad
 *                / fm_repl_apply refuse such a context.  Any other value is FM_ERR_ARG.  fm_loss_grad /
 *                fm_calc_loss_grad stay the reference's squared columns on any context.
 * Zero-initialise the struct: every field's 0 is its default. */
typedef struct fm_config {
  int64_t num_features;
  int32_t k;
  int32_t device;
  uint64_t seed;
  double init_sd;
  double w0;
  int32_t shard_index;
  int32_t shard_count;
  int32_t parallel;
  int32_t n_gpus;
  int32_t devices[FM_MAX_LOCAL];
  int32_t transport;
  int32_t n_procs;
  int32_t proc_rank;
  uint8_t comm_id[128];
  int32_t fuse_single;
  int32_t xchg_chunks;
  int32_t wire;
  int32_t loss;
} fm_config;

/* One mini-batch in CSR form: the result of explode(udfVecToMap(features))
 * (FactorizationMachinesModel.scala:148-153, 244-250).  Row i holds the active entries
 * of sample i (explicit zeros kept, one entry per index).  n_rows counts every sampled
 * row, including rows without active entries: it is miniBatchSize (SGD.scala:124). */
typedef struct fm_csr {
  int64_t n_rows;
  int64_t nnz;
  const int64_t* row_ptr; /* [n_rows + 1], row_ptr[0] == 0 */
  const int32_t* col;     /* [nnz] feature ids */
  const double* val;      /* [nnz] feature values */
  const double* label;    /* [n_rows] */
} fm_csr;

/* What one SGD iteration reports (SGD.scala:134-139 logs lossSum).  loss_sum and n_loss_rows are the
 * context's objective's (fm_config.loss), and so is the loss history. */
typedef struct fm_step_out {
  double loss_sum;      /* sum over samples with >= 1 active entry of (yhat - y)^2 (FM_LOSS_SQUARED) */
  int64_t n_rows;       /* miniBatchSize m */
  int64_t n_loss_rows;  /* samples contributing to loss_sum (FM_LOSS_BPR: (positive, negative) pairs) */
  int64_t n_unique;     /* distinct feature ids touched (U) */
} fm_step_out;

/* ---- context --------------------------------------------------------------------- */
/* Replaces: new FactorizationMachinesModel(uid, k, globalBias, ...) (Model.scala:43-48).
 * A multi-GPU context (parallel != FM_PARALLEL_NONE) accepts every entry point below except the
 * manual fm_shard_* / fm_repl_* phases, fm_set_stream / fm_set_side_stream (unless n_gpus == 1)
 * and fm_loss_grad / fm_calc_loss_grad on a sharded table (FM_ERR_ARG: the per-entry outputs
 * need every owner's rows on one device; replicated contexts answer them); the table entry points
 * act on the rows this process's ranks
 * hold (all rows when n_procs == 1). */
int fm_create(const fm_config* cfg, fm_ctx** out);
/* RCCL unique id for a job of several processes (ncclGetUniqueId), 128 bytes into id. */
int fm_comm_unique_id(uint8_t* id);
void fm_destroy(fm_ctx* ctx);
const char* fm_last_error(void);
/* Launch on an externally owned HIP stream (hipStream_t passed as void*); NULL = the device's
 * default (null) stream.  A new context launches on a non-blocking stream of its own. */
int fm_set_stream(fm_ctx* ctx, void* hip_stream);
/* The context's side stream (hipStream_t as void*), on which batch-only work runs ahead of its
 * step: fm_batch_prepare, fm_shard_route, fm_shard_owner_prepare.  NULL = the context's own
 * non-blocking side stream (the default). */
int fm_set_side_stream(fm_ctx* ctx, void* hip_stream);
/* Wait for everything the context has enqueued: its step stream, its side stream (preparations) and
 * its copy stream (fm_step uploads, fm_batch_from_rows gathers); a multi-GPU context, every rank's. */
int fm_sync(fm_ctx* ctx);
/* Pre-size the per-step workspace (the forward's, the objective stage's, sort's and update's scratch) so that no step on a
 * device-resident batch of at most max_rows x max_nnz allocates.  What belongs to a batch is sized
 * when the batch is first seen, not here: a batch's own prepared view, a multi-GPU context's
 * per-batch routing state and wire buffers, and fm_step's two upload slots, each of which grows to
 * the largest host batch it has held (steady after every batch size has passed through both).  The
 * scratch of fm_rank_candidates / fm_rank_batch is not covered either: it is sized by the two row
 * sets and n_top at the call, and kept; nor are the device copies of the lists of
 * fm_rank_candidates_select / fm_rank_batch_select, sized by U and the lists' total length; nor the
 * scratch of fm_rank_positions / fm_rank_positions_batch: the same row summaries, the device copies of
 * its target and exclude lists and its results, 12 bytes per target; nor the scratch of
 * fm_batch_sample_pairs: the device copies of its lists, the drawn pairs with their labels, lengths and
 * row_ptr (28 bytes per result row) and the scan's per-chunk sums, sized by the largest call.  The
 * _lists forms of these calls (fm_rank_batch_select_lists, fm_rank_positions_batch_lists,
 * fm_batch_sample_pairs_lists) keep no list copies in the context's scratch: they read the fm_lists'
 * own buffers, and the rest of their scratch is the host-list forms'.  Nor is the scratch of
 * fm_binary_metrics / fm_evaluate_binary*: the scores (and fm_binary_metrics' labels), the sort's keys and
 * payloads before and after the re-key, the flags and their scan (44 bytes per row, 52 with the labels), the per-block
 * partials and a sort workspace of the stage's own (24 bytes per row), sized by the largest call. */
int fm_reserve(fm_ctx* ctx, int64_t max_rows, int64_t max_nnz);

/* ---- tables (C9: Strength / FactorizedInteraction, Model.scala:275-289) ------------ */
/* Inject rows (id, w, V[k]) and mark them present: the M0 injection point. */
int fm_load_tables(fm_ctx* ctx, const int32_t* ids, int64_t n, const double* w, const double* V);
/* createInitialModel (SGD.scala:218-252): w, V ~ N(0, init_sd^2) for the given ids,
 * counter-based (seed, id, factor) so the draw is independent of order and shard. */
int fm_init_random(fm_ctx* ctx, const int32_t* ids, int64_t n);
/* Same for every id in [id_begin, id_end) (ids this shard does not own are skipped). */
int fm_init_random_range(fm_ctx* ctx, int64_t id_begin, int64_t id_end);
/* createInitialModel over a device-resident dataset (SGD.scala:224-241: the distinct active ids of
 * the data, then the random draw): every id of the batch's entries that this context owns and
 * that is absent gets the same draw as fm_init_random; present rows are kept.  Runs on the device
 * over the entries (the draw depends on (seed, id, factor) only, so no distinct pass is needed).
 * *n_present (may be NULL) receives the number of present rows afterwards. */
int fm_init_from_batch(fm_ctx* ctx, fm_batch* data, int64_t* n_present);
/* Export every present row owned by this context, ascending id, after applying the
 * pending L1 shrink.  cap = capacity in rows; *n receives the number of present rows
 * (call with cap 0 to size).  V is row-major [n][k]. */
int fm_export_tables(fm_ctx* ctx, int32_t* ids, double* w, double* V, int64_t cap, int64_t* n);
/* The rows of the given ids (each owned by this context) as they stand now, pending L1 shrink
 * applied, without exporting the whole table (the model Datasets queried by id: at F = Int.MaxValue
 * a full export is 2^31 rows).  present[i] = 1 for a present row, else 0 and a zero row.  V is
 * row-major [n][k]. */
int fm_export_rows(fm_ctx* ctx, const int32_t* ids, int64_t n, double* w, double* V, int8_t* present);
int64_t fm_num_present(fm_ctx* ctx);
/* Number of executed (non-empty) SGD steps. */
int64_t fm_epoch(fm_ctx* ctx);

/* ---- mini-batches --------------------------------------------------------------------- */
/* Copy a CSR batch into device memory once (validated: ids in range, row_ptr monotone).
 * A feature id may occur more than once in a row; each occurrence is an entry of its own in the
 * score, the gradients and fm_loss_grad's output, and is counted once in n_unique (fm_step's host
 * batches alike). */
int fm_batch_create(fm_ctx* ctx, const fm_csr* csr, fm_batch** out);
/* Frees the batch's device memory once the work queued on it has run.  A batch may outlive its
 * context, also a multi-GPU context's (fm_destroy drains the context's streams; the batch's
 * destructor touches only its own events and buffers, and a multi-GPU batch points at its context
 * only while it is that context's pending prepare, which fm_destroy clears), but no call takes it
 * after that except this one; a view made by
 * fm_batch_split_view is destroyed before the dataset it borrows from is. */
void fm_batch_destroy(fm_batch* b);
/* Sort the batch's entries by feature (the grouping the gradient reduction consumes) ahead
 * of its step, on the context's side stream, so the sort overlaps whatever the previous step
 * still runs (input prefetch).  The prepared order is consumed by the next fm_step_batch on
 * this batch; a batch that was not prepared is sorted inside its step.  Stream-ordered, no
 * host synchronisation. */
int fm_batch_prepare(fm_ctx* ctx, fm_batch* batch);
/* The mini-batch of the given rows of a device-resident dataset, built on the device: row i of the
 * result is row rows[i] of data (any order, repeats allowed), with its label.  Replaces the split
 * of the cached training data that each SGD iteration consumes -- dfData.cache() and
 * dfData.randomSplit(...) (FactorizationMachinesSGD.scala:93, 111-112): the dataset crosses PCIe
 * once (fm_batch_create), each split is a row list (fm_random_split) gathered on the device.
 * data: a batch of this context made by fm_batch_create (the library keeps its row_ptr on the host
 * too, so the result is sized without a device read; the host pass runs on a pool of host threads).  *out == NULL: a new
 * batch is created; otherwise *out (a batch of this context, not data) is refilled in place.  The
 * gather runs on the context's copy stream behind every queued step, preparation and sharded
 * iteration that reads *out, and the host returns once it is enqueued (rows is copied; the one host
 * wait is for the staging copy of *out's previous refill -- a batch's first refill waits for nothing); steps,
 * fm_batch_prepare, fm_predict_batch and fm_init_from_batch on the result are ordered after it.
 * data must stay alive until the gather has run: fm_sync waits for the context's step, side and
 * copy streams.  A multi-GPU context splits the selected rows contiguously over its local ranks,
 * as fm_batch_create splits a host CSR; each rank gathers its share from its own copy of the
 * dataset (made on its device from the dataset's parts at the first selection). */
int fm_batch_from_rows(fm_ctx* ctx, const fm_batch* data, const int64_t* rows, int64_t n, fm_batch** out);
/* The mini-batch of n (context row, candidate row, label) triples of two device-resident datasets,
 * built on the device: row i of the result holds the entries of row pair_ctx[i] of contexts, in their
 * order, followed by the entries of row pair_cand[i] of candidates, with label[i] -- the row the
 * ranking calls score (fm_rank_candidates), so a recommender trains on the rows it ranks.  Pairs come
 * in any order and may repeat; either row may be empty; the two rows' ids are not checked to be
 * disjoint (an id in both counts as two entries, the ranking calls' rule).  The result is the batch
 * fm_batch_create makes of the host CSR of those concatenated rows -- the same device arrays bit for
 * bit -- so every step, prediction and evaluation on it is that batch's.  contexts, candidates:
 * batches of this context that fm_batch_from_rows accepts as data (their row_ptr is kept on the host;
 * the result's row_ptr is computed there, on the pool of host threads); they may be the same batch.
 * *out as fm_batch_from_rows': NULL creates a batch, otherwise *out (a batch of this context, neither
 * source) is refilled in place, a split view detached first.  An index outside its dataset is
 * FM_ERR_ARG ("pair_ctx ... out of [0, rows of contexts)", "pair_cand ... out of [0, rows of
 * candidates)"); n < 2^31 and fewer than 2^31 result entries.  The lists are copied (pinned staging);
 * the gather runs on the context's copy stream behind every queued step, preparation and sharded
 * iteration that reads *out, and the host returns once it is enqueued, with no host wait but that for
 * *out's own staging.  n = 0 gives an empty batch (its step is FM_NOTHING_TO_DO).  max_id is the
 * larger of the sources'.  The table, the epoch and the histories are untouched.  A multi-GPU context
 * refuses (FM_ERR_ARG: its batches are cut over its ranks). */
int fm_batch_from_pairs(fm_ctx* ctx, const fm_batch* contexts, const fm_batch* candidates,
                        const int32_t* pair_ctx, const int32_t* pair_cand, const double* label,
                        int64_t n, fm_batch** out);
/* The implicit-feedback mini-batch of n_pos positives with n_neg negatives each, drawn on the device:
 * n_pos * (1 + n_neg) rows, row i * (1 + n_neg) the pair (pos_ctx[i], pos_cand[i]) with pos_label, row
 * i * (1 + n_neg) + 1 + j the pair (pos_ctx[i], c_ij) with neg_label, built as fm_batch_from_pairs
 * builds them.  c_ij is drawn uniformly over the candidate rows context u = pos_ctx[i] has not seen:
 * all of [0, C) except its exclude list excl_rows[excl_ptr[u] .. excl_ptr[u + 1]) -- the lists of
 * fm_rank_positions, under the rules of fm_rank_candidates_select's (strictly ascending, in [0, C);
 * messages behind "exclude list: "); excl_ptr == NULL excludes nothing.  The draw is counter-based and
 * part of the contract:
 *   h = splitmix64(seed ^ splitmix64(((uint64)i << 20) | j))
 *   r = ((h >> 32) * E) >> 32            E = C - (length of u's list), 64-bit arithmetic
 *   c_ij = r + #{ t : excl[t] - t <= r }  the r-th eligible row in ascending order
 * so the negatives depend on (seed, i, j), the context's list and C alone -- not on n_pos, the other
 * positives or the launch.  Draws are independent: one positive's negatives may repeat, and a
 * positive whose candidate row is not on its context's list may be drawn as its own negative (put
 * what a context has seen on its list).  0 <= n_neg <= 1024; every context in pos_ctx needs E >= 1
 * (FM_ERR_ARG, "... no eligible candidate row"); all of this is checked on the host before anything is
 * enqueued, and a refused call changes nothing on the device and leaves *out as it was.  n_neg == 0:
 * fm_batch_from_pairs' batch of the positives with a constant label, bit for bit.  sampled (may be
 * NULL): n_pos * n_neg candidate rows, c_ij at [i * n_neg + j].
 * One host wait: the drawn rows' lengths are known on the device alone and the step needs the entry
 * count on the host, so the call reads that total back (8 bytes) and synchronises the copy stream
 * (not the main or the side stream, as fm_shard_route synchronises the side stream alone).  The draw,
 * the lengths, their scan and the read-back run in scratch of the context before *out is waited for
 * or resized; only then is the gather enqueued behind the queued reads of *out -- so a loop that
 * refills two batches in turn never waits for the step in flight.  2^31 or more result entries: FM_ERR_ARG after the
 * read-back, *out untouched.  The lists' device copies, the drawn pairs and the scan's scratch belong
 * to the context and grow to the largest call.  Otherwise as fm_batch_from_pairs (sources, *out,
 * multi-GPU refusal, table untouched). */
int fm_batch_sample_pairs(fm_ctx* ctx, const fm_batch* contexts, const fm_batch* candidates,
                          const int32_t* pos_ctx, const int32_t* pos_cand, int64_t n_pos, int32_t n_neg,
                          const int64_t* excl_ptr, const int32_t* excl_rows,
                          double pos_label, double neg_label, uint64_t seed,
                          fm_batch** out, int32_t* sampled);
/* A training dataset laid out split after split, made resident once: the rows of csr are the
 * randomSplit splits of the cached dfData concatenated in iteration order (FactorizationMachinesSGD
 * .scala:93, 111-112), split s = rows [split_rows[s], split_rows[s + 1]) (split_rows [n_splits + 1],
 * from 0 to n_rows; a last split may hold the rows no iteration samples), each split's rows in the
 * order its mini-batch takes them.  Each split is then a mini-batch in place: fm_batch_split_view
 * hands it to fm_batch_prepare / fm_step_batch with no copy and no gather (fm_batch_from_rows stays
 * for row lists that are not laid out beforehand).  The dataset itself is not stepped or prepared
 * (FM_ERR_ARG; its entries count their sample from their split's first row); fm_init_from_batch
 * (createInitialModel over every row) and fm_batch_from_rows (row i = row i of csr) accept it.  A
 * multi-GPU context cuts every split by rows over its local ranks, as it cuts a host CSR.  Synchronous (returns when the
 * dataset is on the device). */
int fm_batch_create_splits(fm_ctx* ctx, const fm_csr* csr, int32_t n_splits, const int64_t* split_rows,
                           fm_batch** out);
/* The same dataset built from the cached dfData in its own row order
 * (FactorizationMachinesSGD.scala:93, 111-112): csr holds the D = csr->n_rows rows as they were
 * collected, order [n_out] the source row of every laid-out row (row i = row order[i] of csr; any order, repeats allowed, rows may be left out,
 * as the rows of fm_batch_from_rows) and split_rows [n_splits + 1] the split offsets over the laid-out
 * rows (non-decreasing from 0; n_out = split_rows[n_splits] < 2^31, laid-out entries < 2^31).  The
 * source crosses PCIe once in the compact upload form and the device lays it out in one pass (no
 * permuted host copy is made); the result is the dataset fm_batch_create_splits makes of the host CSR
 * of rows order[0 .. n_out) -- the same device arrays bit for bit -- under the same rules (stepped
 * through fm_batch_split_view; accepted by fm_init_from_batch and by fm_batch_from_rows, where row i
 * is laid-out row i).  csr is validated as fm_batch_create validates it; an index of order outside
 * [0, D) is FM_ERR_ARG ("row index out of ...").  A multi-GPU context hands every local rank the
 * source and that rank's share of every split's rows, cut as fm_batch_create_splits cuts them.
 * Synchronous (returns when the dataset is on the device; the source's image is freed by then). */
int fm_batch_layout_splits(fm_ctx* ctx, const fm_csr* csr, int32_t n_splits, const int64_t* split_rows,
                           const int64_t* order, fm_batch** out);
/* Split `split` of a dataset made by fm_batch_create_splits as a mini-batch: its rows, entries and
 * labels where they lie in data (borrowed -- data must outlive the view and every step queued on
 * it).  *out == NULL: a new batch; otherwise *out is re-pointed in place.  Re-pointing a view is
 * host-only, no device work, so a loop re-points the batch it has just stepped while that step still
 * runs (its next fm_batch_prepare waits for it).  The first conversion of a batch that owns device
 * buffers (one made by fm_batch_create or fm_batch_from_rows) into a view blocks: it waits for the
 * batch's queued work, then frees its buffers. */
int fm_batch_split_view(fm_ctx* ctx, const fm_batch* data, int32_t split, fm_batch** out);
/* 1 if a batch prepared by fm_batch_prepare on this context takes the fused step (fm_config.fuse_single
 * and the library's rule: a single-table context, k <= 16, table above 256 MB unless FM_FUSE_ON;
 * multi-GPU contexts never fuse), else 0; -1 for a null context. */
int32_t fm_fuse_active(fm_ctx* ctx);
int64_t fm_batch_rows(const fm_batch* b);
int64_t fm_batch_nnz(const fm_batch* b);
/* The batch's rows per group, read by the FM_LOSS_BPR step alone (fm_config.loss): every `group`
 * consecutive rows are a positive followed by its negatives.  0 = ungrouped.  fm_batch_sample_pairs and
 * fm_batch_sample_pairs_lists set 1 + n_neg on their result (0 with n_neg == 0: no negatives, no groups);
 * every other constructor or refill sets 0 (fm_batch_create, fm_batch_from_rows, fm_batch_from_pairs,
 * fm_batch_split_view).  fm_batch_set_group accepts group == 0, or 2 <= group <= 1025 with n_rows % group
 * == 0; anything else is FM_ERR_ARG, and so are a dataset made by fm_batch_create_splits and a multi-GPU
 * context's batch.  Host-only: nothing is enqueued.  fm_batch_group returns -1 for NULL. */
int fm_batch_set_group(fm_ctx* ctx, fm_batch* batch, int32_t group);
int32_t fm_batch_group(const fm_batch* b);

/* ---- the hot path ------------------------------------------------------------------- */
/* One mini-batch SGD iteration = the foldLeft body, SGD.scala:116-211:
 *   eta = step_size / sqrt(t); lambda = eta * reg_param (SGD.scala:121-122)
 *   forward + loss                      (Model.scala:148-233; SGD.scala:134-138)
 *   per-feature gradient sums           (SGD.scala:142-155; note SURVEY P1: g_w = x*yhat - y)
 *   w -= (sum g_w / m) * eta; V -= (sum g_V) * (eta / m)      (SGD.scala:150-154,171-175)
 *   soft-threshold S_lambda on EVERY present row              (SGD.scala:177-181)
 * t is the 1-based iteration index (tuple._2 + 1, SGD.scala:119).  Returns
 * FM_NOTHING_TO_DO for n_rows == 0 without touching the model (SGD.scala:126-128).
 * fm_step takes the host batch (borrowed for the call only: it is exploded into pinned staging
 * by host threads, then copied asynchronously); fm_step_batch uses a device-resident batch.
 * With out == NULL both only enqueue (no host synchronisation; losses are kept on the device,
 * see fm_loss_history): consecutive fm_step calls then overlap the next batch's host work and
 * copies with the current step (two upload slots used in turn).
 * fm_config.loss: a logistic or BPR context runs its objective stage between the forward and the
 * update.  On an FM_LOSS_BPR context a batch whose group is 0 is FM_ERR_ARG ("... needs a grouped batch
 * ..."; fm_step's host batches always: they carry no group) -- nothing is enqueued, the epoch is
 * unchanged; on other contexts the group is ignored. */
int fm_step(fm_ctx* ctx, const fm_csr* batch, int32_t t, double step_size, double reg_param,
            fm_step_out* out);
int fm_step_batch(fm_ctx* ctx, fm_batch* batch, int32_t t, double step_size,
                  double reg_param, fm_step_out* out);
/* Per-step loss sums of every executed step so far (SGD.scala:139 log line). */
int fm_loss_history(fm_ctx* ctx, double* loss, int64_t cap, int64_t* n);

/* ---- inference & diagnostics ------------------------------------------------------- */
/* FactorizationMachinesModel.transform/predict (Model.scala:69-133): ids absent from the
 * model (or >= num_features) are dropped (inner joins, :103-112); a row with no learned
 * feature gets w0 unclamped (na.fill, :86); otherwise clamp(yhat, min_label, max_label)
 * (:129-132).  Pass -inf/+inf for the unclamped score. */
int fm_predict(fm_ctx* ctx, const fm_csr* csr, double min_label, double max_label, double* pred);
/* The same on a device-resident batch (fm_batch_create): transform over a cached DataFrame
 * without re-uploading it.  pred is a host buffer of fm_batch_rows(batch) doubles. */
int fm_predict_batch(fm_ctx* ctx, fm_batch* batch, double min_label, double max_label, double* pred);
/* Evaluation on the device: the sums RegressionEvaluator / RegressionMetrics take over (prediction,
 * label) -- FactorizationMachinesSample.scala:41-70 drives a CrossValidator over
 * RegressionEvaluator("mae") -- without downloading the predictions.  prediction is fm_predict's value
 * for the row (ids >= num_features or absent dropped, lazy L1 caught up on read, w0 unclamped for a
 * row without a learned entry, else clamp(yhat, min_label, max_label)); the errors e = label -
 * prediction are formed and summed in fp64.  A row without entries is a row: it scores w0 and counts
 * in n_rows and n_unlearned (transform's rule, not the training loss's).
 *   sums  : reduced in a fixed order (per thread, per block, then one fold over the blocks), no
 *           atomics: two evaluations of the same batch on the same table give bitwise equal records.
 *           The order differs from a host sum over the predictions by fp64 rounding only.
 *   labels: the label moments are deliberately not reduced here.  r2's SS_tot formed from sum y and
 *           sum y^2 cancels; the labels are host data wherever a frame exists, so the caller computes
 *           SS_tot there with the two-pass formula, and r2 = 1 - sum_sq_err / SS_tot.
 *   pred  : optional host buffer of n_rows doubles -- transform and evaluate in one pass; the value
 *           stored for a row is the one that was subtracted from its label.
 *   history: every evaluation of a non-empty batch appends one record to the context's evaluation
 *           history (fm_eval_history), which stays on the device until asked for, as the loss
 *           history.  fm_evaluate_batch with out == NULL and pred == NULL only enqueues (no host
 *           synchronisation: a validation curve during a pipelined fit); out == NULL with pred !=
 *           NULL is FM_ERR_ARG.  fm_eval_history waits for the main stream; call it with cap 0 to
 *           size (*n = records so far).
 *   order : on the main stream behind every queued step; a batch refilled by fm_batch_from_rows is
 *           waited for.  The table, the epoch, the loss history and fm_last_stats are unchanged.
 *   arguments : zero rows: FM_NOTHING_TO_DO, *out zeroed, nothing appended.  A dataset made by
 *           fm_batch_create_splits is FM_ERR_ARG (evaluated by split: its split views are accepted).
 *           A null or foreign batch, a null context and the CSR are treated as by fm_predict.
 *   memory: the history starts at 4096 records and doubles; the per-block records and the
 *           synchronous call's device predictions are kept with the context and grow to the largest
 *           call (two equal calls leave fm_device_bytes_live / fm_device_allocs_live equal).
 *   multi-GPU : synchronous only -- out == NULL is FM_ERR_ARG ("a multi-GPU context evaluates
 *           synchronously").  Replicated: every local rank evaluates its part of the batch; sharded:
 *           fm_predict's route -> owner partials -> exchange, ending in the evaluation instead of the
 *           predict epilogue.  The ranks' records are added on the host in local-rank order and kept
 *           in a host-side history that fm_eval_history answers; pred is placed as fm_predict places
 *           it.  With n_procs > 1 a call evaluates this process's rows only, as fm_predict does.  The
 *           manual fm_shard_* phases have no evaluation phase.
 * Profile name: "evaluate" (the kernel and the fold). */
typedef struct fm_eval_out {
  int64_t n_rows;       /* rows evaluated (every row of the batch, empty rows included) */
  int64_t n_unlearned;  /* of those, rows without a learned entry: predicted w0, unclamped */
  int64_t epoch;        /* fm_epoch() when the evaluation was enqueued */
  double sum_err;       /* sum (label - prediction) */
  double sum_abs_err;   /* sum |label - prediction|  -> mae  = / n_rows */
  double sum_sq_err;    /* sum (label - prediction)^2 -> mse, rmse; r2's SS_err */
} fm_eval_out;
int fm_evaluate(fm_ctx* ctx, const fm_csr* csr, double min_label, double max_label, double* pred, fm_eval_out* out);
int fm_evaluate_batch(fm_ctx* ctx, fm_batch* batch, double min_label, double max_label, double* pred,
                      fm_eval_out* out);
int fm_eval_history(fm_ctx* ctx, fm_eval_out* out, int64_t cap, int64_t* n);
/* Binary evaluation on the device: what a click model is chosen by -- log loss and the area under the ROC
 * curve -- and the confusion counts at the threshold score > 0 (sigma(score) > 0.5), from a per-row score
 * and the labels, without downloading the scores.
 *   score : fm_predict's value with the bounds -inf / +inf: the unclamped yhat, w0 for a row without a
 *           learned entry (ids >= num_features or absent dropped, lazy L1 caught up on read).  Whatever
 *           fm_config.loss the context trains with, the score is read as a logit.
 *   label : positive where label > 0.5 (BinaryLabelCounter's rule; 0.5 itself is negative).  The log loss
 *           term softplus(score) - label * score takes the label as given: labels are not checked, and a
 *           fractional label is a soft target there, as in the logistic step.
 *   two_u : twice the Mann-Whitney U of the positives' scores over the negatives': 2 per (positive,
 *           negative) pair the positive wins, 1 per tied pair; AUC = two_u / (2 n_pos n_neg).  Computed in
 *           integers over the fully sorted scores (two stable radix sorts of the scores' 64-bit images, a
 *           scan of the positive flags, one term per run of equal scores): exact, not binned, and bit for
 *           bit reproducible.  -0.0 and +0.0 are one score.  The order of NaN scores is unspecified.
 *           All rows of one class: two_u = 0 (the AUC is undefined: 0 / 0).
 *   sums  : sum_log_loss in fp64, reduced in a fixed order (per thread, per block, one fold), no atomics:
 *           two evaluations of the same batch on the same table give bitwise equal records.
 *   fm_binary_metrics : the same record over n host scores and labels from any model (1 <= n < 2^31; n = 0:
 *           FM_NOTHING_TO_DO, *out zeroed).  Synchronous; appends nothing to the history; epoch = fm_epoch().
 *   fm_evaluate_binary[_batch] : score is an optional host buffer of n_rows doubles, bit for bit
 *           fm_predict[_batch](-inf, +inf)'s.  Every evaluation of a non-empty batch appends one record to
 *           the context's binary evaluation history (fm_eval_binary_history, its own: the regression
 *           history of fm_eval_history is untouched), kept on the device until asked for.
 *           fm_evaluate_binary_batch with out == NULL and score == NULL only enqueues (no host
 *           synchronisation); out == NULL with score != NULL is FM_ERR_ARG.  fm_eval_binary_history waits
 *           for the main stream; call it with cap 0 to size.
 *   order : on the main stream behind every queued step; a batch refilled by fm_batch_from_rows is
 *           waited for.  The table, the epoch, the loss history, the regression evaluation history and
 *           fm_last_stats are unchanged.
 *   arguments : zero rows: FM_NOTHING_TO_DO, *out zeroed, nothing appended.  A dataset made by
 *           fm_batch_create_splits is FM_ERR_ARG (its split views are accepted).  A null or foreign batch
 *           is FM_ERR_ARG.  Any single-table context is accepted, whatever its loss; a multi-GPU context
 *           or shard_count > 1 is FM_ERR_ARG (the message names the call).
 *   memory: the history starts at 4096 records of 64 bytes and doubles; the scratch (scores, keys, flags,
 *           scan arrays, a sort workspace of the stage's own) is kept with the context and grows to the
 *           largest call: two equal calls leave fm_device_bytes_live / fm_device_allocs_live equal.
 * Profile names: "evaluate_binary" (the score pass through the fold), and inside it "binary_sort" and
 * "binary_count" (the flags' scan, the pair count, the fold). */
typedef struct fm_binary_out {
  int64_t n_rows;   /* rows evaluated; n_neg = n_rows - n_pos */
  int64_t n_pos;    /* rows with label > 0.5 */
  int64_t epoch;    /* fm_epoch() when the evaluation was enqueued */
  int64_t tp;       /* score > 0 among the positives */
  int64_t fp;       /* score > 0 among the negatives */
  int64_t two_u;    /* AUC = two_u / (2 n_pos n_neg) */
  double sum_log_loss; /* sum softplus(score) - label * score -> logLoss = / n_rows */
} fm_binary_out;
int fm_binary_metrics(fm_ctx* ctx, const double* score, const double* label, int64_t n, fm_binary_out* out);
int fm_evaluate_binary(fm_ctx* ctx, const fm_csr* csr, double* score, fm_binary_out* out);
int fm_evaluate_binary_batch(fm_ctx* ctx, fm_batch* batch, double* score, fm_binary_out* out);
int fm_eval_binary_history(fm_ctx* ctx, fm_binary_out* out, int64_t cap, int64_t* n);
/* Top-N ranking, the serving side of transform (the shape of ALSModel.recommendForUserSubset): for
 * every row of `contexts` (a user and their history, a page view) the n_top rows of `candidates`
 * (movies, ads) with the largest FM score of the two rows' entries taken together, without
 * materialising the U x C concatenated rows.  top_index[u * n_top + j] = the candidate row ranked
 * j-th for context u, top_score[u * n_top + j] = its score (host buffers of U * n_top).
 *   score : fm_predict's for the row made of the two entry lists, one after the other: ids >=
 *           num_features or absent from the model are dropped (Model.scala:103-112), the lazy L1
 *           shrink is caught up on read, a pair with no learned entry on either side scores w0
 *           unclamped (Model.scala:86), every other pair clamp(yhat, min_label, max_label)
 *           (:129-132).  An id that occurs in both rows counts as two entries (the library does not
 *           check that the two rows are disjoint).  Labels are not read.
 *   order : by the unclamped yhat, descending (a pair with no learned entry ranks at w0); equal keys
 *           by ascending candidate row.  So the result is a function of the two row sets and the
 *           table alone: not of the library's tiling, of U, or of the other contexts in the call.
 *           top_score holds the clamped value, which may tie where the order does not.  The order
 *           of NaN keys is unspecified.
 *   arithmetic : yhat(u, c) = w0 + a_u + b_c + <S_u, S_c> with S_r = sum v x, a_r = b_r = sum w x +
 *           (|S_r|^2 - sum |v|^2 x^2) / 2 per row: fp64 sums of the fp32 table values, the pair term
 *           an fp64 dot product in a fixed factor order; nothing on the path is rounded to fp32.
 *   arguments : 1 <= n_top <= min(C, FM_RANK_MAX_TOP), else FM_ERR_ARG; C = 0 with U >= 1 is
 *           FM_ERR_ARG; U = 0 is FM_OK with nothing written; C < 2^31; null pointers are FM_ERR_ARG;
 *           the CSRs are validated as fm_predict validates its own.
 *   contexts : a single table with shard_count == 1; a replicated multi-GPU context is answered by
 *           its first rank (fm_rank_candidates only: its batches are cut over the ranks, so
 *           fm_rank_batch is FM_ERR_ARG there).  A row-sharded table (FM_PARALLEL_SHARDED, or
 *           shard_count > 1) is FM_ERR_ARG: left for later, and natural there -- the per-owner row
 *           summaries are additive, and the fp64 wire of the sharded step (FM_WIRE_FP64) already
 *           carries exactly these words.
 * Synchronous, on the context's main stream behind every queued step; the table, the epoch and the
 * loss history are unchanged.  The scratch is kept with the context and grows to the largest call
 * (two equal calls leave fm_device_bytes_live / fm_device_allocs_live equal). */
#define FM_RANK_MAX_TOP 1024
int fm_rank_candidates(fm_ctx* ctx, const fm_csr* contexts, const fm_csr* candidates, int32_t n_top,
                       double min_label, double max_label, int32_t* top_index, double* top_score);
/* The same on device-resident batches of this context (fm_batch_create / fm_batch_from_rows /
 * fm_batch_split_view results; a split dataset itself is FM_ERR_ARG, as for fm_step_batch); waits
 * for a refilled batch's gather. */
int fm_rank_batch(fm_ctx* ctx, fm_batch* contexts, fm_batch* candidates, int32_t n_top,
                  double min_label, double max_label, int32_t* top_index, double* top_score);
/* Ranking within per-context candidate lists: context u carries a list of candidate rows,
 * sel_rows[sel_ptr[u] .. sel_ptr[u + 1]), and ranks only those rows (FM_RANK_SELECT_ONLY: second-stage
 * ranking of a retrieval's candidates out of one shared pool) or every row except those
 * (FM_RANK_SELECT_EXCEPT: top-N unseen; the exclusion happens before the selection, so n_top results
 * survive it).  FM_RANK_SELECT_ALL ignores the lists (they may be NULL) and is fm_rank_candidates /
 * fm_rank_batch, bit for bit.
 *   lists : host arrays.  sel_ptr has U + 1 entries, sel_ptr[0] == 0, non-decreasing, sel_ptr[U] <
 *           2^31; a list's entries are candidate rows in [0, C), strictly ascending.  The host checks
 *           all of it in one pass before anything is enqueued; a violation is FM_ERR_ARG with the
 *           context and the position in fm_last_error() ("... ascending ...", "... out of range ...",
 *           "sel_ptr ...", "select ...", "null ..."), and a refused call changes nothing on the device.
 *   score, order : an eligible pair's key and score are fm_rank_candidates' for that pair, bit for bit;
 *           ties go to the ascending candidate row.  A context's result depends on the rows, the table
 *           and its own list alone.
 *   fewer eligible rows than n_top : the eligible rows come first, in order; the remaining slots hold
 *           top_index = -1 and top_score = NaN (a context with nothing eligible: all of them).  n_top
 *           keeps its rule, 1 <= n_top <= min(C, FM_RANK_MAX_TOP), whatever the lists hold.
 *   cost : FM_RANK_SELECT_EXCEPT scores all U x C pairs, as the unrestricted call; FM_RANK_SELECT_ONLY
 *           scores the listed pairs alone (work proportional to the list lengths).
 * Everything else as fm_rank_candidates / fm_rank_batch: U = 0, C = 0, null pointers, the CSRs, batches
 * of another context, split datasets, a replicated group (host rows only, answered by its first
 * rank), a row-sharded table (FM_ERR_ARG), synchronous on the main stream, nothing of the context's
 * state changed.  The device copies of the lists are scratch of the context like the rest and grow to
 * the largest call. */
#define FM_RANK_SELECT_ALL 0     /* lists ignored (may be NULL): fm_rank_candidates' result, bit for bit */
#define FM_RANK_SELECT_ONLY 1    /* context u ranks only the candidate rows of its list */
#define FM_RANK_SELECT_EXCEPT 2  /* context u ranks every candidate row except those of its list */
int fm_rank_candidates_select(fm_ctx* ctx, const fm_csr* contexts, const fm_csr* candidates, int32_t select,
                              const int64_t* sel_ptr, const int32_t* sel_rows, int32_t n_top,
                              double min_label, double max_label, int32_t* top_index, double* top_score);
int fm_rank_batch_select(fm_ctx* ctx, fm_batch* contexts, fm_batch* candidates, int32_t select,
                         const int64_t* sel_ptr, const int32_t* sel_rows, int32_t n_top,
                         double min_label, double max_label, int32_t* top_index, double* top_score);
/* Exact rank positions, the evaluation side of ranking: where do a context's held-out rows land among
 * everything it has not seen?  Context u's targets are the candidate rows tgt_rows[tgt_ptr[u] ..
 * tgt_ptr[u + 1]), its excluded rows (what it rated in training) excl_rows[excl_ptr[u] .. excl_ptr[u + 1]);
 * excl_ptr == NULL excludes nothing (excl_rows is then ignored).  For e over tgt_rows (host buffers of
 * tgt_ptr[U] elements):
 *   position[e] : the 0-based position of that target in the context's order over its eligible rows --
 *           all candidate rows except its excluded ones: the number of eligible rows that rank before
 *           it.  The key and the order are fm_rank_candidates': the unclamped yhat descending, a pair
 *           without a learned entry at w0, ties by ascending candidate row.  Exact for any C (a count,
 *           not a sort: nothing is limited by FM_RANK_MAX_TOP), and a sum of integers, so equal calls
 *           give equal bits.  The order of NaN keys is unspecified.
 *   score[e] : what top_score holds for the pair: the clamped value, w0 unclamped where nothing is learned.
 *   a target that is itself excluded : position -1, score NaN; the other targets are not affected.
 *   the defining property : for every target with 0 <= position[e] < n_top,
 *           fm_rank_*_select(FM_RANK_SELECT_EXCEPT, the same exclude lists, n_top) -- with excl_ptr ==
 *           NULL the unrestricted call -- returns that row at top_index[u * n_top + position[e]] with
 *           top_score equal to score[e] bit for bit.
 *   lists : both obey the _select list rules (offsets from 0, non-decreasing, below 2^31; rows in [0, C),
 *           strictly ascending per list), checked in one pass before anything is enqueued, with the same
 *           messages behind "target list: " or "exclude list: " and the arguments' names (tgt_ptr,
 *           excl_ptr, ...).  tgt_ptr == NULL is FM_ERR_ARG.  A refused call changes nothing on the
 *           device.
 * U = 0 is FM_OK with nothing written, and so is tgt_ptr[U] == 0 (valid lists, no target).  Everything
 * else as fm_rank_candidates / fm_rank_batch: C = 0 with U >= 1 and C >= 2^31 are FM_ERR_ARG, null
 * pointers, the CSRs, batches of another context, split datasets, a replicated group (host rows only,
 * answered by its first rank), a row-sharded table (FM_ERR_ARG), synchronous on the main stream behind
 * every queued step; the table, the epoch, the loss and evaluation histories and fm_last_stats are
 * unchanged.  The lists' device copies and the results are scratch of the context like the rest and
 * grow to the largest call. */
int fm_rank_positions(fm_ctx* ctx, const fm_csr* contexts, const fm_csr* candidates, const int64_t* tgt_ptr,
                      const int32_t* tgt_rows, const int64_t* excl_ptr, const int32_t* excl_rows,
                      double min_label, double max_label, int32_t* position, double* score);
int fm_rank_positions_batch(fm_ctx* ctx, fm_batch* contexts, fm_batch* candidates, const int64_t* tgt_ptr,
                            const int32_t* tgt_rows, const int64_t* excl_ptr, const int32_t* excl_rows,
                            double min_label, double max_label, int32_t* position, double* score);
/* ---- resident row lists --------------------------------------------------------------------
 * The per-context candidate-row lists that fm_rank_batch_select (sel), fm_rank_positions_batch (tgt, excl)
 * and fm_batch_sample_pairs (excl) take, kept on the device: built once, read by every later call.  The
 * host-list forms check, stage and upload their lists at every call (a training loop hands over every
 * context's exclude list at every mini-batch); the _lists forms below take an fm_lists instead and do no
 * host check, staging or upload of list rows.
 * An fm_lists holds U lists over C candidate rows: device int64 ptr[U + 1] and int32 rows[ptr[U]], each list
 * strictly ascending and in [0, C), with a host copy of ptr and the longest list's length.  It belongs to
 * the context that made it, is read-only afterwards, and counts in fm_device_bytes_live /
 * fm_device_allocs_live with its two buffers.  0 <= U, C < 2^31.  A multi-GPU context refuses both
 * constructors (FM_ERR_ARG), as it refuses the batch forms of the calls that read the lists.
 *   fm_lists_create : from host arrays under fm_rank_candidates_select's list rules, checked in one pass
 *           with the same messages behind "row lists: " and the argument names ptr / rows.  Synchronous; a
 *           refused call allocates nothing that stays and leaves *out as it was.
 *   fm_lists_from_pairs : from n (context, candidate) pairs, on the device: context u's list is the distinct
 *           pair_cand[i] with pair_ctx[i] == u, ascending -- what a training loop's interactions say each
 *           context has seen.  Pairs come in any order and may repeat; a context without a pair gets an
 *           empty list; n = 0 gives U empty lists; n < 2^31.  An index outside [0, U) / [0, C) is FM_ERR_ARG
 *           ("pair_ctx index out of [0, U = ...)", "pair_cand index out of [0, C = ...)"), checked on the pool
 *           of host threads before anything is enqueued.  Two stable radix sorts (by candidate, then by
 *           context), head flags of the runs of equal pairs, their scan, one binary search per offset and a
 *           compaction: integer work, no atomics, so equal inputs -- in any order -- give equal bytes.
 *           Synchronous, on the main stream behind every queued step; it reads ptr back once (the host copy,
 *           the longest list, and the size of rows).  Its scratch (the pairs' upload, the sorts' buffers, the
 *           flags, the scan's arrays) is the call's own and freed before it returns: afterwards the live bytes
 *           have grown by the object's two buffers and nothing else.
 *   fm_lists_destroy : frees at once.  Every consumer below has finished reading the lists when it returns:
 *           the rank calls are synchronous, and fm_batch_sample_pairs_lists waits for its draw on the copy
 *           stream -- the gather it leaves queued reads the drawn pairs, not the lists.  A later consumer that
 *           leaves a read of the lists queued must add an event for this call to wait for.  Lists may outlive
 *           their context; no call takes them after that except this one.
 *   fm_lists_contexts / _candidates / _total / _longest : U, C, ptr[U] and the longest list (-1 for NULL).
 *   fm_lists_export : the device arrays back on the host: ptr [U + 1] and rows [fm_lists_total], either may
 *           be NULL; cap_rows (the capacity of rows) below the total is FM_ERR_ARG.  Synchronous. */
int fm_lists_create(fm_ctx* ctx, int64_t U, int64_t C, const int64_t* ptr, const int32_t* rows, fm_lists** out);
int fm_lists_from_pairs(fm_ctx* ctx, int64_t U, int64_t C, const int32_t* pair_ctx, const int32_t* pair_cand,
                        int64_t n, fm_lists** out);
void fm_lists_destroy(fm_lists* lists);
int64_t fm_lists_contexts(const fm_lists* lists);
int64_t fm_lists_candidates(const fm_lists* lists);
int64_t fm_lists_total(const fm_lists* lists);
int64_t fm_lists_longest(const fm_lists* lists);
int fm_lists_export(fm_ctx* ctx, const fm_lists* lists, int64_t* ptr, int32_t* rows, int64_t cap_rows);
/* fm_rank_batch_select, fm_rank_positions_batch and fm_batch_sample_pairs with their lists resident: the
 * same paths, the device pointers taken from the objects instead of from an upload, so the results are
 * the host-list calls' with the same lists, bit for bit (-1 / NaN slots, excluded targets, sampled and
 * the batch's device arrays included).  sel may be NULL with FM_RANK_SELECT_ALL only; tgt must not be
 * NULL; excl == NULL excludes nothing (the host calls' excl_ptr == NULL).  FM_ERR_ARG, each with a message
 * that names the mismatch: lists of another context, lists whose U or C differ from the batches' row
 * counts.  The sampled call's E >= 1 rule reads the object's host copy of ptr.  Everything else -- arguments,
 * order, synchronisation, refusals, U = 0, no target -- as the host-list call. */
int fm_rank_batch_select_lists(fm_ctx* ctx, fm_batch* contexts, fm_batch* candidates, int32_t select,
                               const fm_lists* sel, int32_t n_top, double min_label, double max_label,
                               int32_t* top_index, double* top_score);
int fm_rank_positions_batch_lists(fm_ctx* ctx, fm_batch* contexts, fm_batch* candidates, const fm_lists* tgt,
                                  const fm_lists* excl, double min_label, double max_label, int32_t* position,
                                  double* score);
int fm_batch_sample_pairs_lists(fm_ctx* ctx, const fm_batch* contexts, const fm_batch* candidates,
                                const int32_t* pos_ctx, const int32_t* pos_cand, int64_t n_pos, int32_t n_neg,
                                const fm_lists* excl, double pos_label, double neg_label, uint64_t seed,
                                fm_batch** out, int32_t* sampled);
/* calcLossGrad (Model.scala:135-234), per active entry e in CSR order:
 * pred[e] = yhat of its row (unclamped), loss[e] = (yhat - y)^2, delta_w[e] = x,
 * delta_v[e*k + f] = vfxiSum_f * x - (v_f * x) * x.  Any output may be NULL.
 * Ids absent from the model are an error here (the reference fills them with an
 * unseeded random draw, Model.scala:170-171, which is never reached from fit).  The reference's
 * squared columns on any context, whatever its fm_config.loss. */
int fm_loss_grad(fm_ctx* ctx, const fm_csr* csr, double* pred, double* loss, double* delta_w,
                 double* delta_v);
/* calcLossGrad(dfSampleIndexed, initialSd) with the reference's fill for ids the model lacks
 * (Model.scala:144-146, 170-171: coalesce(strength, randn() * initialSd) and udfInitVec() per
 * joined row): every entry whose id is absent (or >= num_features) gets its own w and v drawn
 * from N(0, initial_sd^2) -- keyed by (seed, entry index in CSR order, column), so a call is
 * reproducible where the reference's draws are unseeded.  initial_sd must be > 0 (:136).
 * Refused on a row-sharded multi-GPU context (see fm_create). */
int fm_calc_loss_grad(fm_ctx* ctx, const fm_csr* csr, double initial_sd, uint64_t seed, double* pred,
                      double* loss, double* delta_w, double* delta_v);
/* VectorSum UDAF + groupBy (FactorizationMachines.scala:45-81): for every distinct key,
 * the element-wise fp64 sum of its k-vectors in input order.  Output ascending by key;
 * *n_out = number of distinct keys (<= n).  Runs the device sort + segmented reduction. */
int fm_vector_sum_by_key(fm_ctx* ctx, const int32_t* keys, int64_t n, const double* vecs,
                         int32_t k, int32_t* out_keys, double* out_sums, int64_t* n_out);

/* Per-kernel device time of the last fm_step_batch calls, measured with HIP events on the
 * launch stream when enabled (names: "forward", "sort", "update", ...). */
int fm_profile_enable(fm_ctx* ctx, int32_t on);
/* Writes up to cap entries: names as a '\n'-joined string into names (size names_cap),
 * total milliseconds and launch counts per kernel; *n = number of kernels. */
int fm_profile_read(fm_ctx* ctx, char* names, int64_t names_cap, double* total_ms,
                    int64_t* launches, int64_t cap, int64_t* n);
int fm_profile_reset(fm_ctx* ctx);
/* Device memory the library holds right now, over every context, batch and device of the process:
 * bytes and number of live allocations (every device allocation of the library is counted; exact,
 * no context, no host synchronisation).  A steady-state call leaves both unchanged; destroying every
 * context and batch returns both to 0. */
int64_t fm_device_bytes_live(void);
int64_t fm_device_allocs_live(void);

/* ---- input format: Spark 2.1 `libsvm` data source (data/sample.txt, config c1) ------------ */
/* MLUtils.parseLibSVMFile semantics: trimmed lines, '#'-lines and empty lines skipped, one-based
 * strictly ascending indices (stored 0-based), numFeatures = max last index + 1 (an empty row
 * counts as index 0).  Call with cap_rows = cap_nnz = 0 to size: *n_rows, *nnz, *num_features
 * are always filled; then again with buffers label[n_rows], row_ptr[n_rows + 1], col[nnz],
 * val[nnz].  A malformed line is an FM_ERR_ARG with the line in fm_last_error(). */
int fm_read_libsvm(const char* path, int64_t cap_rows, int64_t cap_nnz, double* label, int64_t* row_ptr,
                   int32_t* col, double* val, int64_t* n_rows, int64_t* nnz, int64_t* num_features);

/* ---- mini-batch sampler: Dataset.randomSplit replay (SGD.scala:111-112) --------------- */
/* Host-side replay of Spark 2.1.0 randomSplit(weights, seed) on a cached DataFrame whose
 * rows are given partition by partition (part_ptr[n_parts+1]).  Each partition is sorted
 * ascending by all columns in schema order (column_order: 'L' label double, 'F' features
 * vector, 'I' int64 column extra[] ; sampleId is appended last), then split i keeps the
 * rows whose XORShiftRandom(seed + partition).nextDouble() falls in
 * [cumw[i], cumw[i+1]).  Features: vec_type (0 sparse, 1 dense), vec_size,
 * vec_ptr[n+1], vec_idx (sparse only; ignored for dense), vec_val.
 * Outputs: split_of[n] (-1 = in no split), sample_id[n] = (partition << 33) + row index
 * (monotonically_increasing_id, Model.scala:268-272), order[n] = row indices in sorted
 * (per-partition) order.  Partitions are sorted and sampled in parallel on the library's host
 * thread pool (each writes only its own rows; the result does not depend on the thread count);
 * an allocation failure is FM_ERR_OOM. */
int fm_random_split(int32_t n_parts, const int64_t* part_ptr, const char* column_order,
                    const double* label, const int8_t* vec_type, const int32_t* vec_size,
                    const int64_t* vec_ptr, const int32_t* vec_idx, const double* vec_val,
                    const int64_t* extra, int32_t n_weights, const double* weights,
                    int64_t seed, int32_t* split_of, int64_t* sample_id, int64_t* order);
/* The building blocks, exported for the parity tests. */
int64_t fm_xorshift_hash_seed(int64_t seed);
int32_t fm_murmur3_bytes_hash(const uint8_t* data, int64_t len, int32_t seed);
/* n successive nextDouble() of XORShiftRandom(seed). */
int fm_xorshift_next_doubles(int64_t seed, int64_t n, double* out);

/* ---- row-sharded multi-GPU step (owner-computes) -----------------------------------------
 * One context per rank (fm_config.shard_index / shard_count = rank / R, R <= 64; the owner of
 * feature id is id % R, its local slot id / R).  The caller exchanges the device buffers
 * between phases with all-to-all (RCCL over xGMI; fm_spark_amd/distributed.py).  Replaces the
 * feature-keyed shuffles S1/S2/S5/S6 and the per-sample window of the reference plan
 * (Model.scala:155-164, :191, SGD.scala:148-166).
 * A "pair" is (sample of a source rank, owner holding some of its entries).  Wire buffers are
 * structures of arrays over P pairs, kp + 2 words per pair (kp = roundup(k, 4)):
 *   partials = [P][kp] sum v*x, then [P][2] {sum v^2 x^2, sum w*x}; words of the context's
 *              fm_config.wire: fp32 (FM_WIRE_FP32: 4 (kp + 2) P bytes) or fp64 (FM_WIRE_FP64:
 *              8 (kp + 2) P bytes, the scalar section at byte 8 kp P).  This is the size of
 *              partials_out (P = sum src_pairs) and of partials_in (P = sum counts[R..2R)).
 *   S        = [P][kp] vfxiSum, then [P][2] {r, yhat}  (the residual r = yhat - y is formed in fp64
 *              from the fp64 label, as the reference's Double column, SGD.scala:145-146, and rounded
 *              once; the owner forms g_w = x*yhat - y as (x - 1)*yhat + r); always fp32, 4 (kp + 2) P
 *              bytes: s_send / s_recv do not depend on fm_config.wire (they are the values the single
 *              table's update reads)
 * so the exchange is two all-to-alls per direction (the vector section, the scalar section).
 * The phases are the squared step's: each refuses a context whose fm_config.loss is not FM_LOSS_SQUARED.
 * Every phase is keyed by `batch`, this rank's mini-batch of the iteration; its state lives with
 * the batch.  Phases 1 and 1b depend on the batch alone and run on the side stream
 * (fm_set_side_stream), so the next iteration's routing, entry exchange and slot sort overlap the
 * current iteration; phases 2-4 run on the main stream and wait for them through events.
 * Phase 1 (requester): partition the batch's entries by owner, CSR order kept, into
 * send_slot (uint32 local slots, N) and send_ent ({index of the entry's (sample, owner) pair
 * among this rank's pairs to that owner, x bits}, N) -- device buffers of the batch's nnz.
 * counts[0..R) = entries to each owner, counts[R..2R) = pairs to each owner.
 * Synchronises the side stream (not the main stream). */
int fm_shard_route(fm_ctx* ctx, fm_batch* batch, void* send_slot, void* send_ent, int64_t* counts);
/* Phase 1b (owner): the n received entries (source-rank major: src_entries[r] from rank r, which
 * sent src_pairs[r] pairs) -> their pair table and their order by slot (stable: source rank,
 * then CSR order), kept with `batch`.  No host synchronisation.  recv_slot / recv_ent must stay
 * valid until the main stream has run fm_shard_owner_forward of this batch. */
int fm_shard_owner_prepare(fm_ctx* ctx, fm_batch* batch, const void* recv_slot, const void* recv_ent,
                           int64_t n, const int64_t* src_entries, const int64_t* src_pairs);
/* Phase 2 (owner): partials_out[sum src_pairs] (source-major, sample order): per received pair
 * the partial forward sums over the entries this rank owns, lazy L1 caught up on read; fp32 or fp64
 * words as this context's fm_config.wire says (above). */
int fm_shard_owner_forward(fm_ctx* ctx, fm_batch* batch, void* partials_out);
/* Phase 3 (requester): the partials received from the owners (owner-major, counts[R + o] rows
 * from owner o; words of this context's fm_config.wire) -> per sample S, yhat and the loss; s_send
 * gets the S rows in the same layout, fp32. */
int fm_shard_combine(fm_ctx* ctx, fm_batch* batch, const void* partials_in, void* s_send);
/* Phase 4 (owner): the S rows received for its pairs (same order as its partials) -> per-slot
 * gradient sums over the slot-sorted entries, update + L1 with global miniBatchSize global_rows
 * (the sum of every rank's rows).  Returns FM_NOTHING_TO_DO when global_rows == 0 (every rank
 * skips, SGD.scala:126-128). */
int fm_shard_owner_update(fm_ctx* ctx, fm_batch* batch, const void* s_recv, int32_t t, double step_size,
                          double reg_param, int64_t global_rows);

/* ---- replicated multi-GPU step (small tables) --------------------------------------------
 * Every rank holds the whole table (shard_count = 1, same seed / same loaded tables) and steps
 * its own rows of the global mini-batch.
 * Phase 1: forward, sort and per-slot gradient sums of this rank's batch into the device
 * buffer grad[num_features][kp + 4] fp32 = [sum g_V (kp) | sum g_w | touched | 0] (zeroed
 * first; an empty batch contributes zeros and returns FM_NOTHING_TO_DO).
 * The caller all-reduces grad (sum; RCCL over xGMI), then
 * Phase 2: the update + L1 of SGD.scala:150-181 on every touched row with global miniBatchSize
 * global_rows; identical on every rank, so the replicas stay identical.  Returns
 * FM_NOTHING_TO_DO when global_rows == 0. */
int fm_repl_grad(fm_ctx* ctx, fm_batch* batch, void* grad);
int fm_repl_apply(fm_ctx* ctx, const void* grad, int32_t t, double step_size, double reg_param,
                  int64_t global_rows);

/* Statistics of the last step on this context: loss sum and loss rows of its samples, distinct
 * ids (sharded: those this rank owns; replicated: touched rows of the whole step).  Multi-GPU
 * callers all-reduce the first two (SGD.scala:134-139). */
int fm_last_stats(fm_ctx* ctx, double* loss_sum, int64_t* n_loss_rows, int64_t* n_unique);

#ifdef __cplusplus
}
#endif

#endif /* FM_HIP_H */
