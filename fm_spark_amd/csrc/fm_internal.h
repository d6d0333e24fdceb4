// Internal declarations shared by the HIP translation units of libfm_hip.so.
// Nothing here crosses the C-ABI (include/fm_hip.h).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fm_hip.h"

namespace fmhip {

// ------------------------------------------------------------------------ errors
void set_error(const std::string& msg);

struct Error {
  int code;
  std::string msg;
};

#define FM_HIP_CHECK(expr)                                                            \
  do {                                                                                \
    hipError_t _e = (expr);                                                           \
    if (_e != hipSuccess)                                                             \
      throw ::fmhip::Error{_e == hipErrorOutOfMemory ? FM_ERR_OOM : FM_ERR_HIP,        \
                           std::string(#expr) + ": " + hipGetErrorString(_e)};        \
  } while (0)

#define FM_REQUIRE(cond, msg)                                \
  do {                                                       \
    if (!(cond)) throw ::fmhip::Error{FM_ERR_ARG, (msg)};    \
  } while (0)

// -------------------------------------------------------------------- device table
// Per feature row, one record aligned to a 64- or 128-byte line so that a random row access
// costs one line (random gathers on MI355X are bound by 128-byte line requests):
//   float V[kp]          kp = roundup(k, 4); padding columns stay exactly 0 through updates
//   RowHdr {w, t, cum}   at float offset kp (16-byte aligned)
//   t   : epoch (executed steps) through which the row is current; -1 = absent
//   cum : sum of lambda over executed steps 1..t, i.e. the L1 shrink already applied.
// A row read at epoch E is brought current by S_{cum[E] - cum} (lazy L1, see fm_device.h).
struct alignas(16) RowHdr {
  float w;
  int32_t t;
  double cum;
};

struct TableView {
  float* rec;      // [rows * stride]
  int64_t rows;    // local rows
  int32_t k;
  int32_t kp;
  int32_t stride;  // record stride in floats (16 or 32, or a multiple of 32)
  int32_t shard_count;
  int32_t shard_index;
  __host__ __device__ float* v(int64_t slot) const { return rec + slot * stride; }
  __host__ __device__ RowHdr* hdr(int64_t slot) const {
    return reinterpret_cast<RowHdr*>(rec + slot * stride + kp);
  }
};

// record stride (floats) for k factors: the smallest 64 B / 128 B line that holds V + header,
// else a multiple of 128 B
inline int32_t record_stride(int32_t kp) {
  const int32_t need = kp + 4;
  if (need <= 16) return 16;
  if (need <= 32) return 32;
  return (need + 31) / 32 * 32;
}

// device buffer: owns its allocation (freed by the destructor; move-only), or borrows a range of
// another buffer (a view: never freed here).  Every device allocation of the library is one of
// these, counted in fm_device_bytes_live / fm_device_allocs_live.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  bool borrowed = false;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes), borrowed(o.borrowed) {
    o.p = nullptr;
    o.bytes = 0;
    o.borrowed = false;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      bytes = o.bytes;
      borrowed = o.borrowed;
      o.p = nullptr;
      o.bytes = 0;
      o.borrowed = false;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  // n bytes at q inside a buffer someone else owns (what this one owned is freed)
  void borrow(const void* q, size_t n) {
    release();
    p = const_cast<void*>(q);
    bytes = n;
    borrowed = true;
  }
  void ensure(size_t n);
  // at least n bytes; a growth takes an eighth more (batches refilled with slightly different
  // sizes, e.g. randomSplit splits, then stop growing: a growth drains the device)
  void ensure_slack(size_t n) {
    if (n > bytes || !p) ensure(n + n / 8 + 4096);
  }
  void release();
  template <class T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

// ------------------------------------------------------------------- radix sort
struct SortWork {
  DevBuf keys_a, keys_b, vals_a, vals_b, counts, digit_tot;
  int64_t cap = 0;
  void ensure(int64_t n);
};

// Stable LSD sort of (key, index) pairs: keys_in[n] (uint32, < 2^key_bits) with payload
// = original index (vals_in == nullptr) or vals_in[n].  Returns pointers to the sorted
// keys / payloads (inside `w`).
void radix_sort_pairs(SortWork& w, const uint32_t* keys_in, const uint32_t* vals_in, int64_t n,
                      int key_bits, hipStream_t st, const uint32_t** keys_out,
                      const uint32_t** vals_out);
// Same with an 8-byte payload (e.g. the exploded entry {sample, x}).  When final_keys /
// final_vals are given, the last pass writes there (a batch's own sorted view).
void radix_sort_pairs64(SortWork& w, const uint32_t* keys_in, const uint2* vals_in, int64_t n,
                        int key_bits, hipStream_t st, const uint32_t** keys_out,
                        const uint2** vals_out, uint32_t* final_keys = nullptr,
                        uint2* final_vals = nullptr);
// Stable sort by key bits [lo_bit, hi_bit) only (the bits below ride along), output written to
// final_keys / final_vals.  The keys must hold nothing at hi_bit and above (fm_shard_route's end at
// sb + ob): the last pass takes a whole digit, so such bits would be sorted on as well
// (tests/test_gpu_sort.py test_sort_by_a_bit_range).
void radix_sort_pairs64_bits(SortWork& w, const uint32_t* keys_in, const uint2* vals_in, int64_t n, int lo_bit,
                             int hi_bit, hipStream_t st, uint32_t* final_keys, uint2* final_vals);

// ---------------------------------------------------------------- step kernels
// (fm_forward.hip, fm_update.hip, fm_table.hip, fm_batch.hip)
// A device-resident mini-batch: the exploded (sampleId, featureId, featureValue) rows of
// Model.scala:148-153 kept both as CSR (row_ptr) and as COO entries ent[e] = {sample, x bits}.
struct BatchDev {
  int64_t n_rows = 0, nnz = 0;
  DevBuf row_ptr, col, ent, label;  // int64 [B+1], uint32 [N] feature slot, uint2 [N], double [B]
  DevBuf xs;                         // fp32 [N]: x alone, the forward's stream (8 B per entry with col)
};
// The byte size of each BatchDev buffer for B rows and N entries.  The kernels read past the end on
// purpose (k_forward's unguarded loads from clamped indices: at least 4 entries and 16 bytes beyond),
// so this padding is a safety condition, and every constructor of a batch sizes its buffers here.
struct BatchBytes {
  size_t row_ptr, col, ent, xs, label;
};
inline BatchBytes batch_bytes(int64_t B, int64_t N) {
  const size_t n = (size_t)(N > 4 ? N : 4), b = (size_t)(B > 4 ? B : 4);
  return {sizeof(int64_t) * (size_t)(B + 1), sizeof(uint32_t) * n + 16, sizeof(uint2) * n + 16, sizeof(float) * n + 16,
          sizeof(double) * b + 16};
}
// d holds B rows and N entries: its five buffers grown (never shrunk) to batch_bytes, with slack
inline void size_batch(BatchDev& d, int64_t B, int64_t N) {
  const BatchBytes z = batch_bytes(B, N);
  d.n_rows = B;
  d.nnz = N;
  d.row_ptr.ensure_slack(z.row_ptr);
  d.col.ensure_slack(z.col);
  d.ent.ensure_slack(z.ent);
  d.xs.ensure_slack(z.xs);
  d.label.ensure_slack(z.label);
}

// The single-table step's per-sample record: S (kp floats) and, for kp <= 16, the sample's
// {r, yhat} in the same 64-B (kp <= 12) or 128-B (kp = 16) record, so the update's S gather and
// {r, yhat} load hit one line; wider rows keep {r, yhat} in StepWork::yl.
inline bool s_rec_yl(int kp) { return kp <= 16; }
inline int s_rec_floats(int kp) { return s_rec_yl(kp) ? (kp + 2 <= 16 ? 16 : 32) : kp; }

struct StepWork {
  DevBuf S;         // [B * kp] float: per-sample vfxiSum
  DevBuf yl;        // [B] float2 {r, yhat}: r = yhat - y formed in fp64 from the fp64 label, then rounded
  DevBuf loss_part; // [n_fwd_blocks] double2 {loss, n_loss}
  DevBuf part;      // [ceil(N / 256) * 2 * (kp+2)] double partial gradients (one range per update wave)
  DevBuf ucnt;      // [n_update_blocks] uint32 distinct-id counts per block
  DevBuf eval_part; // [n_eval_blocks][kEvalRec] double: an evaluation's per-block records (grown to the largest launch)
  SortWork sort;
};

// where sample s's {r, yhat} lies during a single-table step: yl[s * stride], inside the S record
// (s_rec_yl) or in StepWork::yl -- the addresses launch_forward writes and launch_segment_update reads
struct StepYl {
  float2* yl;
  int64_t stride;  // in float2 elements
};
inline StepYl step_yl(const StepWork& w, int kp) {
  if (s_rec_yl(kp)) return {reinterpret_cast<float2*>(w.S.as<float>() + kp), (int64_t)s_rec_floats(kp) / 2};
  return {w.yl.as<float2>(), 1};
}

struct StepParams {
  int64_t n_rows;
  double eta;        // stepSize / sqrt(t)
  double lam;        // eta * regParam
  double scale_v;    // eta / m
  double m;          // miniBatchSize as double: (sum / m) * eta
  int32_t epoch;     // steps executed before this one (E)
  double cumE;       // cum[E]
  double cum_next;   // cum[E] + lam = cum[E+1]
  double w0;
};

// k_forward's modes (fm_forward.hip): the step's forward, plain or with the singleton rows' updates
// fused in; the sharded owner's partial pass with the fp32 or the fp64 wire; predict (clamp bounds,
// fp64 score per sample into pred); calcLossGrad (fp64 pred / loss / dw per entry, dv [entries][k],
// the absent-id flag); a row's fp64 summary for ranking (predict's entry handling, the fp64 partial
// pass's stores: S, {sum v^2 x^2, sum w x} and the learned-entry count per row); evaluation (predict's
// score of every row reduced against its fp64 label into one kEvalRec record per block, and stored as
// well if pred is given)
enum FwdMode : int {
  kTrain = 0, kPartial = 1, kPredict = 2, kLossGrad = 3, kTrainFused = 4, kPartial64 = 5, kSummary = 6, kEvaluate = 7
};
// doubles of an evaluation record: {rows, rows without a learned entry, sum e, sum |e|, sum e^2},
// e = label - prediction (fm_device.h, EvalAcc)
constexpr int kEvalRec = 5;
struct FwdOut {
  int mode = kTrain;  // a FwdMode; launch_forward sets the partial modes itself (partial_out / partial_wide)
  double lo = 0.0, hi = 0.0;
  double* pred = nullptr;  // kEvaluate: optional (the prediction that was subtracted from the label)
  double* loss = nullptr;
  double* dw = nullptr;
  double* dv = nullptr;
  int32_t* absent = nullptr;
  uint32_t* pcount = nullptr;  // partial pass (sharded predict): present rows per pair; kSummary: learned entries per row
  double* summary = nullptr;   // kSummary: [rows][kp] doubles sum v*x, then [rows] double2 {sum v^2 x^2, sum w*x}
  // partial pass over chunk ch_c of ch_C (ch_C > 1): of every source r < ch_R, the pairs
  // [off[r] + P_r ch_c / ch_C, off[r] + P_r (ch_c + 1) / ch_C), P_r = off[r + 1] - off[r] (device off)
  const int64_t* ch_off = nullptr;
  int32_t ch_R = 0, ch_c = 0, ch_C = 1;
  // loss-grad mode: fill_sd > 0 gives an entry whose id the model lacks its own N(0, fill_sd^2)
  // w and v draws (calcLossGrad's coalesce with randn / udfInitVec, Model.scala:144-146,170-171),
  // keyed by (fill_seed, entry index, column)
  double fill_sd = 0.0;
  uint64_t fill_seed = 0;
  // kTrainFused: the forward applies the update of every row whose header carries no multi tag of
  // this epoch (a singleton; fm_device.h "Singleton rows"), with sp (set by the launch); kp <= 16
  StepParams sp{};
};
constexpr int kMaxChunkSources = 64;  // sources a chunked partial pass can split
// partial_out != nullptr: the sharded owner's partial pass (fm_shard.hip): [pairs][kp] fp32 vectors
// followed by [pairs] float2 scalars (pred->pcount, if given: present rows per pair); partial_wide:
// the fp64 wire, [pairs][kp] doubles followed by [pairs] double2, at the same address;
// else pred != nullptr: FactorizationMachinesModel.predict / calcLossGrad (p.w0, p.cumE used)
void launch_forward(const TableView& T, const BatchDev& b, StepWork& w, const StepParams& p,
                    hipStream_t st, int64_t* n_fwd_blocks, float* partial_out = nullptr,
                    const FwdOut* pred = nullptr, bool partial_wide = false);
// A seam for the suite (tests/native/forward_probe.hip), not configuration: a process-wide cap on the
// forward's blocks in place of the tuned constant, so a test can make every team walk several
// samples at a batch of a few hundred rows.  0 (the default) = the tuned grid.  It is not in
// include/fm_hip.h and is not read from the environment.  While a cap is set, every forward launch
// of the process (the step, the fused step, predict, loss-grad, each rank's partial passes) is
// appended to a bounded log (the first kFwdLogCap launches since the last clear); with no cap set
// nothing is logged and a launch costs one relaxed load.
struct FwdLaunchRec {
  int32_t mode, gs, team, u;  // the k_forward instantiation: FwdMode, lanes per row, lanes per sample, passes in flight
  int32_t chunk, chunks;      // the partial pass's chunk (0 of 1 elsewhere): the launch walks that chunk's pairs only
  int64_t blocks, rows;       // the grid launched, and the batch's rows (all the owner's pairs, for a partial pass)
};
constexpr int kFwdLogCap = 256;
struct FwdConsts {
  int32_t grid, block, fuse_ns, fuse_u;  // the tuned block cap, threads per block, kFuseNS, kFuseU
};
void set_forward_grid_cap(int64_t blocks);
void clear_forward_log();
int read_forward_log(FwdLaunchRec* out, int cap);  // copies at most cap records; returns the launches under a cap since the last clear
FwdConsts forward_consts();

// per-sample inputs of the segmented update: S rows of s_stride floats, {yhat, y} at yl[s * yl_stride]
struct SegSource {
  const float* S;
  int64_t s_stride;
  const float2* yl;
  int64_t yl_stride;
  // non-null: the entry count is n_dev[0] (device) <= N, and n_dev[1] singleton rows were updated
  // by the fused forward (added to the distinct count)
  const int64_t* n_dev = nullptr;
};
// emit != nullptr (replicated mode): the per-slot gradient sums go to emit[rows][kp + 4] as
// [sum g_V (kp) | sum g_w | 1 (touched) | 0] instead of being applied to the table
void launch_segment_update(const TableView& T, const BatchDev& b, StepWork& w, const StepParams& p,
                           const uint32_t* skeys, const uint2* sents, int64_t n_fwd_blocks,
                           double* stats_out, hipStream_t st, float* emit = nullptr, const int64_t* n_dev = nullptr);
// The objective stage (fm_objective.hip), between launch_forward and launch_segment_update of a step
// whose context's loss is FM_LOSS_LOGISTIC or FM_LOSS_BPR (group: the batch's rows per group, BPR only;
// it divides b.n_rows): every sample's {r, yhat} becomes {r, r} with the objective's r, computed in fp64
// from the stored fp32 yhat, and w.loss_part gets the stage's own per-block {loss, loss rows}.  Returns
// the number of those partials (<= kLossPartBlocks), which launch_segment_update takes in place of the
// forward's block count.
int64_t launch_objective(int32_t loss, int32_t group, int kp, const BatchDev& b, StepWork& w, hipStream_t st);
// the fused step's singleton split of a prepared sorted view, at the step (fm_update.hip; fm_device.h
// "Singleton rows"): the entries of runs of two or more, in order, into mkeys / ments (capacity N); n_out[0] =
// their count, n_out[1] = the number of singleton runs (device); each multi run's row in tag_T gets
// the epoch's multi tag
struct SplitWork {
  DevBuf cnt, off;
};
void launch_split(const uint32_t* skeys, const uint2* sents, int64_t N, SplitWork& sw, uint32_t* mkeys, uint2* ments,
                  int64_t* n_out, hipStream_t st, const TableView& tag_T, int32_t epoch);
void launch_segment_update(const TableView& T, int64_t N, const SegSource& src, StepWork& w, const StepParams& p,
                           const uint32_t* skeys, const uint2* sents, int64_t n_loss_blocks, double* stats_out,
                           hipStream_t st, float* emit = nullptr);
// A seam for the suite (tests/native/update_probe.hip), not configuration: the update side's
// geometry at padded width kp, read from the constants and the kp -> kernel choice that
// launch_segment_update and launch_split use, so a test can place runs of equal keys against
// the kernels' boundaries without keeping a copy of them.  No kernel reads it.
struct UpdGeometry {
  int32_t wave_entries;       // sorted entries per update wave (= per combine range)
  int32_t group_entries;      // entries per lane group of k_segment_update at this kp
  int32_t block_entries;      // entries per update block
  int32_t paired;             // 1: a run closed in phase 2 leaves in a paired row store at this kp (table mode)
  int32_t comb_lanes;         // k_segment_combine's lanes per range
  int32_t comb_cols;          // long-run columns a combine lane sums at once
  int32_t split_chunk;        // sorted entries per split wave
  int32_t scan_round_chunks;  // split chunks k_split_scan takes per round
};
UpdGeometry update_geometry(int kp);
// The same kind of seam for the sharded step's own kernels (fm_shard.hip; tests/native/shard_probe.hip):
// the sizes at which a route, pair-table, combine or pack kernel takes another tile, trip or grid-stride
// sweep, read from the constants its launches use.  No kernel reads it.
struct ShardGeometry {
  int32_t pair_tile;       // samples per tile of the pair numbering (k_pair_count / k_pair_index: one block)
  int32_t route_team;      // lanes per sample of k_sample_mask
  int64_t mask_sweep;      // samples one grid-stride sweep of k_sample_mask takes
  int32_t scan_trip;       // tiles one trip of k_rows_scan takes
  int64_t route_sweep;     // entries one sweep of k_route_keys takes at unroll step 0 (u >= 1 starts beyond them)
  int32_t route_unroll;    // entries a k_route_keys thread takes per sweep
  int64_t table_sweep;     // the same of k_pair_table
  int32_t table_unroll;
  int32_t slot_regs;       // up to this many owners the combine keeps a sample's pair slots in registers
  int32_t max_r;           // the most ranks
  int32_t combine_team;    // at this kp: lanes per sample of k_shard_combine / predict / evaluate
  int64_t combine_sweep;   // at this kp: samples one grid-stride sweep of them takes
  int64_t pack_sweep;      // at this kp: pairs one sweep of k_pack_srec takes (0: no packed record at this kp)
};
ShardGeometry shard_geometry(int kp);
// replicated mode: apply the all-reduced gradient sums grad[rows][kp + 4] to every touched row;
// the number of touched rows -> *n_touched (device, fp64 stats slot), through per-block counts in
// blk_touched[kReplApplyBlocks]
constexpr int kReplApplyBlocks = 256 * 16;
// The most blocks that leave a loss partial (StepWork::loss_part is reserved for this many): the
// grid cap of the sharded combine.  The single-table forward sizes loss_part by its own grid.
constexpr int kLossPartBlocks = 256 * 8;
void launch_repl_apply(const TableView& T, const float* grad, const StepParams& p, uint32_t* blk_touched,
                       double* n_touched, hipStream_t st);

void launch_init_random(const TableView& T, const int32_t* ids, int64_t n, int64_t id_begin,
                        uint64_t seed, double sd, int32_t epoch, double cumE, hipStream_t st);
void launch_load_rows(const TableView& T, const int32_t* ids, int64_t n, const double* w,
                      const double* V, int32_t epoch, double cumE, hipStream_t st);
void launch_flush(const TableView& T, int32_t epoch, double cumE, hipStream_t st);
void launch_gather_rows(const TableView& T, const int32_t* ids, int64_t n, double cumE, double* w, double* V,
                        int8_t* present, hipStream_t st);
void launch_table_reset(const TableView& T, hipStream_t st);
void launch_predict(const TableView& T, const BatchDev& b, double cumE, double w0, double lo, double hi,
                    double* pred, hipStream_t st);
// fm_evaluate*: predict's score of every row against its label, reduced on the device.  The forward
// (team shapes and entry handling of launch_predict; b.n_rows > 0) leaves one record per block in
// w.eval_part and returns the number of blocks; launch_eval_fold sums the n_blocks records of a launch
// (of the forward, or of the sharded requester's k_shard_evaluate) into out[kEvalRec] (device): one
// block, thread t the records t, t + kBlock, ... in order, then the block reduction -- an order that
// depends on n_blocks alone.  pred (device, optional): the predictions.  No atomics: equal inputs give
// equal bits.
int64_t launch_evaluate(const TableView& T, const BatchDev& b, StepWork& w, double cumE, double w0, double lo, double hi,
                        double* pred, hipStream_t st);
void launch_eval_fold(const double* part, int64_t n_blocks, double* out, hipStream_t st);
// fm_rank_*: every row's summary (FwdOut::summary's layout) and its count of learned entries, with
// predict's team shapes; ids outside the table or absent from the model contribute nothing
void launch_summary(const TableView& T, const BatchDev& b, double cumE, double* summary, uint32_t* present,
                    hipStream_t st);
void launch_init_entries(const TableView& T, const uint32_t* col, int64_t n, uint64_t seed, double sd,
                         int32_t epoch, double cumE, hipStream_t st);
void launch_loss_grad(const TableView& T, const BatchDev& b, double cumE, double w0, double* pred,
                      double* loss, double* dw, double* dv, int32_t* absent_flag, hipStream_t st,
                      double fill_sd = 0.0, uint64_t fill_seed = 0);
void launch_segment_sum(const uint32_t* skeys, const uint32_t* svals, int64_t n, const double* vecs,
                        int32_t k, uint32_t* run_index, int32_t* out_keys, double* out_sums,
                        int64_t* n_out_dev, hipStream_t st);
void launch_count_present(const TableView& T, int64_t* out, hipStream_t st);
// the uploaded CSR image (row_ptr, label, xoff, col with bit 31 = a value follows, the compact
// non-unit values), on the host (the pinned staging) or on the device (its copy)
struct CsrImage {
  int64_t* row_ptr;
  double* label;
  int32_t* xoff;
  uint32_t* col;
  float* x;
};
// the device image -> the device batch: row_ptr / label / col copied, ent[e] = {sample of e, x
// bits} rebuilt from row_ptr and the compact values (the explode of Model.scala:148-153)
void launch_explode(const CsrImage& in, int64_t B, int64_t N, BatchDev& dst, hipStream_t st);
// fm_batch_layout_splits: the device image of the source (as launch_explode takes it) -> dst
// row s = source row order[s] (device order[B]), laid out split after split: row_ptr_in[B + 1]
// (device) is the result's row_ptr, computed by the host; split_rows [n_splits + 1] (device);
// split_rp [B + n_splits] and the entries' sample indices as launch_split_rebase leaves them
void launch_layout_splits(const CsrImage& src, const int64_t* order, const int64_t* row_ptr_in, const int64_t* split_rows,
                          int32_t n_splits, int64_t B, BatchDev& dst, int64_t* split_rp, hipStream_t st);

// ---------------------------------------------------------------- ranking (fm_rank.hip)
// Scratch of fm_rank_candidates / fm_rank_batch, kept with the context (grown, never shrunk).
struct RankWork {
  DevBuf sum_u, sum_c;    // the two row sets' summaries (FwdOut::summary's layout)
  DevBuf cnt_u, cnt_c;    // uint32 learned entries per row
  DevBuf bias_u, bias_c;  // double a_r = L + (|S|^2 - Q) / 2 per row
  DevBuf lkey, lidx;      // the context tile's split lists: uint64 keys, uint32 candidate rows
  DevBuf out_idx, out_score;  // int32 / double [U][n_top]
  DevBuf sel_ptr, sel_rows;   // fm_rank_*_select: the call's lists, int64 [U + 1] offsets and int32 candidate rows
                              // (fm_rank_positions: its exclude lists)
  DevBuf tgt_ptr, tgt_rows;   // fm_rank_positions: the target lists, laid out as sel_ptr / sel_rows
  DevBuf position, pos_score;  // ... and its results, int32 / double per target
};
// a call's per-context row lists (validated): ptr[U + 1], rows[ptr[U]] on the host; ptr null: no list.
// dev_ptr set: the lists of an fm_lists, resident already -- ptr is the object's host copy of the offsets,
// rows stays null, and the call neither stages nor uploads anything of them.
struct RankList {
  const int64_t* ptr = nullptr;
  const int32_t* rows = nullptr;
  int64_t longest = 0;  // the longest list of the call
  const int64_t* dev_ptr = nullptr;
  const int32_t* dev_rows = nullptr;
};
// one row set's per-row arrays on the device: the summaries (FwdOut::summary's layout), a_r and the
// learned entries of n rows
struct RankSide {
  const double* sum;
  const double* bias;
  const uint32_t* cnt;
  int64_t n;
  // rows [r0, r0 + nt) of it: a context tile
  RankSide tile(int64_t r0, int64_t nt, int kp) const { return {sum + r0 * kp, bias + r0, cnt + r0, nt}; }
};
// candidate splits of a call of U contexts (whole chunks each; fewer as the contexts alone fill the
// chip) and the contexts one pass of the score kernel takes (the list budget)
int rank_splits(int64_t C, int64_t U);
int64_t rank_ctx_tile(int splits, int n_top);
// a_r for n rows of a summary buffer
void launch_rank_bias(const double* summary, int64_t n, int kp, double* bias, hipStream_t st);
// the contexts u (a tile) against all candidates c: per (context, split) the split's best n_top in order
// into lkey / lidx [u.n][splits][n_top].  select FM_RANK_SELECT_ALL: every candidate, the lists not read.
// Else under per-context lists (device: sel_ptr[u.n + 1] of this tile, offsets into sel_rows; rows in
// [0, c.n), strictly ascending per list).  FM_RANK_SELECT_EXCEPT: a listed row enters as padding, the
// splits cut the candidates as without lists.  FM_RANK_SELECT_ONLY: the splits (rank_splits of the call's
// longest list) cut each context's list; a split without a chunk writes n_top padding entries.
void launch_rank_score(int select, const RankSide& u, const RankSide& c, const int64_t* sel_ptr, const int32_t* sel_rows,
                       int kp, int splits, int n_top, double w0, uint64_t* lkey, uint32_t* lidx, hipStream_t st);
// the splits' lists merged in split order; the first n_top per context into out_idx / out_score
// (w0 for a pair without a learned entry, else the key's value clamped to [lo, hi]; row -1 and NaN
// where a list's entry is padding: fewer eligible rows than n_top)
void launch_rank_merge(const uint64_t* lkey, const uint32_t* lidx, int64_t Ut, int splits, int n_top,
                       const uint32_t* cnt_u, const uint32_t* cnt_c, double w0, double lo, double hi, int32_t* out_idx,
                       double* out_score, hipStream_t st);
// fm_rank_positions: the contexts u (a tile of at most rank_position_ctx_tile()) against all candidates c.
// Device lists as launch_rank_score takes them: tgt_ptr[u.n + 1] / tgt_rows, the longest of the tile's
// target lists `longest` >= 1; ex_ptr / ex_rows the exclude lists, ex_ptr null for
// none.  Per target e the rows of this launch's splits that rank before it are added onto position[e]
// (zeroed by the caller; integer atomics) and score[e] is written: k_rank_merge's score of the pair;
// -1 / NaN for a target on its context's exclude list.
int64_t rank_position_ctx_tile();
void launch_rank_position(const RankSide& u, const RankSide& c, const int64_t* tgt_ptr, const int32_t* tgt_rows,
                          int64_t longest, const int64_t* ex_ptr, const int32_t* ex_rows, int kp, int splits, double w0,
                          double lo, double hi, int32_t* position, double* score, hipStream_t st);

// fm_batch_from_rows: dst row s = src row rows[s] (device rows[B]); row_ptr_in[B + 1] (device) is the
// result's row_ptr, computed by the host from the source's
void launch_select_rows(const BatchDev& src, const int64_t* rows, const int64_t* row_ptr_in, int64_t B, BatchDev& dst,
                        hipStream_t st);
// ---------------------------------------------------------------- pair batches (fm_pairs.hip)
// Scratch of fm_batch_sample_pairs, kept with the context (grown, never shrunk) and touched on the copy
// stream alone (fm_pairs.hip's header).
struct PairWork {
  DevBuf lists;                // the call's lists: int64 excl_ptr [U + 1], then int32 pos_ctx, pos_cand [n_pos], excl_rows
                               // (fm_batch_sample_pairs_lists: the positives alone, the exclude lists are the fm_lists')
  DevBuf pair_ctx, pair_cand;  // int32 [B]: every output row's pair
  DevBuf label;                // double [B]
  DevBuf len;                  // uint32 [B]: every output row's entries
  DevBuf row_ptr;              // int64 [B + 1]: their exclusive scan
  DevBuf chunk_tot, chunk_off;  // int64 per scan chunk
  DevBuf total;                // int64 [1]: the result's entries, read back by the host
};
// fm_batch_from_pairs / fm_batch_sample_pairs: dst row s = contexts row pair_ctx[s] followed by candidates
// row pair_cand[s] (device lists [B]); row_ptr_in [B + 1] and label_in [B] (device) are the result's
void launch_pair_rows(const int32_t* pair_ctx, const int32_t* pair_cand, const int64_t* row_ptr_in, const double* label_in,
                      const BatchDev& contexts, const BatchDev& candidates, int64_t B, BatchDev& dst, hipStream_t st);
// chunks of the row_ptr scan over B rows (the size of chunk_tot / chunk_off)
int64_t pair_scan_chunks(int64_t B);
// the exclusive scan of len[B] (uint32) into off[B + 1] (int64; off[B] = the sum, also left in total[0]) by
// the three phases k_pair_chunk_sum / k_pair_scan_chunks / k_pair_scan_rows; chunk_tot / chunk_off hold
// pair_scan_chunks(B) int64 each.  B = 0: off[0] = total[0] = 0.  fm_batch_sample_pairs' row_ptr and
// fm_lists_from_pairs' offsets (fm_lists.hip) are both this scan.
void launch_len_scan(const uint32_t* len, int64_t B, int64_t* off, int64_t* chunk_tot, int64_t* chunk_off, int64_t* total,
                     hipStream_t st);
// fm_batch_sample_pairs' device side before the gather: the B = n_pos (1 + n_neg) pairs (each positive,
// then its drawn negatives; device lists, excl_ptr null for none), their labels and lengths, row_ptr
// [B + 1] by the three-phase scan and total[0] = row_ptr[B]
void launch_pair_sample(const int32_t* pos_ctx, const int32_t* pos_cand, int64_t n_pos, int32_t n_neg, const int64_t* excl_ptr,
                        const int32_t* excl_rows, double pos_label, double neg_label, uint64_t seed, const BatchDev& contexts,
                        const BatchDev& candidates, int32_t* pair_ctx, int32_t* pair_cand, double* label, uint32_t* len,
                        int64_t* row_ptr, int64_t* chunk_tot, int64_t* chunk_off, int64_t* total, hipStream_t st);

// ---------------------------------------------------------------- resident row lists (fm_lists.hip)
// fm_lists_from_pairs' device side, in two halves around the one read-back (ptr: it sizes rows).  Both take
// the n pairs sorted by (context, candidate) -- sctx / scand, device, as two stable radix sorts leave them.
// launch_lists_offsets: flag[i] = 1 where sorted pair i opens a (context, candidate) run, off[n + 1] = the
// flags' exclusive scan (launch_len_scan; total[0] = the distinct pairs), ptr[v] = off[the first sorted pair
// with context >= v] for v in [0, U].  launch_lists_compact: a flagged pair i writes rows[off[i]] = scand[i].
// Integer work, one writer per slot, no atomics: equal inputs give equal bytes.
void launch_lists_offsets(const uint32_t* sctx, const uint32_t* scand, int64_t n, int64_t U, uint32_t* flag, int64_t* off,
                          int64_t* chunk_tot, int64_t* chunk_off, int64_t* total, int64_t* ptr, hipStream_t st);
void launch_lists_compact(const uint32_t* scand, const uint32_t* flag, const int64_t* off, int64_t n, int32_t* rows,
                          hipStream_t st);

// ---------------------------------------------------------------- binary evaluation (fm_binary.hip)
// int64 words of a binary evaluation record on the device (one 64-byte line): {n_rows, n_pos, tp, fp, two_u,
// the bits of sum_log_loss, 0, 0}
constexpr int kBinaryRec = 8;
// Scratch of fm_binary_metrics / fm_evaluate_binary*, kept with the context (grown to the largest call, never
// shrunk) and used on the main stream alone.  The sort workspace is the stage's own: the context's other
// workspaces may be sorting a prepared batch on the side stream.
struct BinaryWork {
  DevBuf score, label;      // double [n]: the scores (launch_predict's, or fm_binary_metrics' upload) / its labels
  DevBuf key_lo, pay;       // uint32 [n] low key words, uint2 [n] {high key word, positive flag}: the first sort's input
  DevBuf key_hi, pay2;      // the same re-keyed: the second sort's input
  DevBuf flag, cp;          // uint32 [n] sorted positive flags, int64 [n + 1] their exclusive scan
  DevBuf chunk_tot, chunk_off, total;  // launch_len_scan's
  DevBuf rows_part, count_part;        // the per-block partials of k_binary_rows / k_binary_count
  DevBuf rec;               // int64 [kBinaryRec]: fm_binary_metrics' record (the evaluations write into the history)
  SortWork sort;
  const uint32_t* sorted_hi = nullptr;  // the second sort's output (inside `sort`), valid from launch_binary_sort
  const uint2* sorted_pay = nullptr;    // until the next one
  void ensure(int64_t n);  // everything but score / label / rec, for n rows
};
// The stage in three launches, so that a profile can tell them apart; n in [1, 2^31), score / label device [n]:
// the per-row pass (its partials and the sort's input), the two stable sorts, then the flags' scan, the pair
// count and the fold of both partials into rec[kBinaryRec] (device).
void launch_binary_rows(BinaryWork& w, const double* score, const double* label, int64_t n, hipStream_t st);
void launch_binary_sort(BinaryWork& w, int64_t n, hipStream_t st);
void launch_binary_count(BinaryWork& w, int64_t n, int64_t* rec, hipStream_t st);

// fm_batch_create_splits: each split's own row_ptr (rebased to its first entry) into split_rp
// [B + n_splits] and every entry's sample index made relative to its split's first row
// (split_rows [n_splits + 1], device)
void launch_split_rebase(const BatchDev& b, const int64_t* split_rows, int32_t n_splits, int64_t* split_rp,
                         hipStream_t st);

}  // namespace fmhip
