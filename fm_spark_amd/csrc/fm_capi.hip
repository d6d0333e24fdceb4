// C-ABI implementation of include/fm_hip.h: contexts, device tables, mini-batch upload,
// the step driver (forward -> sort -> segmented update) and the table import/export.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <set>
#include <thread>
#include <utility>

#include "fm_context.h"
#include "fm_hostpool.h"

namespace fmhip {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

void report_stale(hipError_t e) {
  if (e == hipSuccess) return;
  static std::mutex mu;
  static std::set<int> seen;
  std::lock_guard<std::mutex> lk(mu);
  if (seen.insert((int)e).second)
    fprintf(stderr, "[libfm_hip] cleared a stale HIP error left by an earlier call: %d %s\n", (int)e, hipGetErrorString(e));
}

// live device memory of the process (fm_device_bytes_live / fm_device_allocs_live): every device
// allocation of the library is a DevBuf, so these two are exact
static std::atomic<int64_t> g_dev_bytes_live{0}, g_dev_allocs_live{0};

void DevBuf::ensure(size_t n) {
  if (n <= bytes && p && !borrowed) return;
  // growing: work already queued on any stream may still read the old buffer (asynchronous
  // steps), so the device drains before it is freed
  if (p && !borrowed) FM_HIP_CHECK(hipDeviceSynchronize());
  release();
  if (n == 0) n = 16;
  FM_HIP_CHECK(hipMalloc(&p, n));
  bytes = n;
  g_dev_bytes_live.fetch_add((int64_t)n, std::memory_order_relaxed);
  g_dev_allocs_live.fetch_add(1, std::memory_order_relaxed);
}

void DevBuf::release() {
  if (p && !borrowed) {
    (void)hipFree(p);
    g_dev_bytes_live.fetch_sub((int64_t)bytes, std::memory_order_relaxed);
    g_dev_allocs_live.fetch_sub(1, std::memory_order_relaxed);
  }
  p = nullptr;
  bytes = 0;
  borrowed = false;
}

// How many contiguous chunks parallel_chunks cuts [0, n) into (one per pool thread, at least
// min_per_thread items each).
static int64_t chunk_count(int64_t n, int64_t min_per_thread) {
  return std::max<int64_t>(1, std::min<int64_t>(HostPool::get().threads(), n / std::max<int64_t>(min_per_thread, 1)));
}

// f(t, lo, hi) for chunk t = [n t / T, n (t + 1) / T) of T chunks, on the pool's threads.
template <class F>
static void parallel_chunks_t(int64_t n, int64_t T, F&& f) {
  if (T <= 1) {
    f(int64_t(0), int64_t(0), n);
    return;
  }
  const std::function<void(int)> job = [&](int t) { f((int64_t)t, n * t / T, n * (t + 1) / T); };
  HostPool::get().run((int)T, job);
}

// f(lo, hi) over [0, n) in contiguous chunks on the pool's threads; small ranges run inline.
template <class F>
static void parallel_chunks(int64_t n, int64_t min_per_thread, F&& f) {
  parallel_chunks_t(n, chunk_count(n, min_per_thread), [&](int64_t, int64_t lo, int64_t hi) { f(lo, hi); });
}

// rows[n] of a dataset of Bd rows (hrp: its host row_ptr) -> hrows[n] (the rows, copied) and rp[n + 1],
// the selection's own row_ptr; false when a row is outside [0, Bd).  Random reads of the dataset's
// row_ptr, about 2 ms for 256K rows on one thread -- longer than the GPU step -- so on the pool's
// threads: each chunk's running lengths, then the chunks' offsets.
static bool selection_row_ptr(const int64_t* hrp, int64_t Bd, const int64_t* rows, int64_t n, int64_t* hrows,
                              int64_t* rp) {
  rp[0] = 0;
  const int64_t T = chunk_count(n, 8192);
  std::vector<int64_t> tot(T + 1, 0);
  std::atomic<int> bad{0};
  parallel_chunks_t(n, T, [&](int64_t t, int64_t lo, int64_t hi) {
    int64_t acc = 0;
    for (int64_t i = lo; i < hi; ++i) {
      const int64_t r = rows[i];
      if (r < 0 || r >= Bd) {
        bad.store(1);
        return;
      }
      hrows[i] = r;
      acc += hrp[r + 1] - hrp[r];
      rp[i + 1] = acc;
    }
    tot[t + 1] = acc;
  });
  if (bad.load()) return false;
  for (int64_t t = 0; t < T; ++t) tot[t + 1] += tot[t];  // the chunks' offsets
  if (T > 1)
    parallel_chunks_t(n, T, [&](int64_t t, int64_t lo, int64_t hi) {
      const int64_t add = tot[t];
      if (add)
        for (int64_t i = lo; i < hi; ++i) rp[i + 1] += add;
    });
  return true;
}

// Host CSR -> pinned staging [row_ptr int64 B+1][label f64 B][xoff int32 B][col u32 N][x f32 N]:
// values that round to 1.0f (one-hot / categorical fields) are not sent -- the id's bit 31 (free:
// ids are non-negative int32) marks an entry whose fp32 value follows in the x area, and xoff[i]
// is where row i's values start; each host thread packs its rows' values from its first entry's
// position on, and only those runs are copied -- so 4 B per unit entry and 8 B per other entry
// cross PCIe.  The device rebuilds each entry's sample index and value (k_explode) into the exploded
// {sample, x} entries of Model.scala:148-153.  Validated on the way; host threads write the
// staging directly.  check_range: ids must be owned by this context's table (training); otherwise
// any non-negative int32 id is accepted (predict drops unknown ids).
struct Staged {
  int64_t B = 0, N = 0, M = 0, max_id = -1, max_len = 0;
  size_t o_lab = 0, o_xoff = 0, o_col = 0, o_x = 0, bytes = 0;  // bytes: the image through col
  size_t o_extra = 0;  // the caller's `extra` bytes of staging, behind the x area
  int nruns = 0;
  int64_t run_at[16] = {0}, run_n[16] = {0};  // packed value runs in the x area (floats)
  // the image's five arrays at base: the pinned staging, or its device copy
  CsrImage view(void* base) const {
    char* p = reinterpret_cast<char*>(base);
    return {reinterpret_cast<int64_t*>(p), reinterpret_cast<double*>(p + o_lab), reinterpret_cast<int32_t*>(p + o_xoff),
            reinterpret_cast<uint32_t*>(p + o_col), reinterpret_cast<float*>(p + o_x)};
  }
  // the image's copies from the staging to its device copy, on st: one through col, then the packed
  // value runs, each where its rows' xoff point
  void enqueue_copies(void* dev, const void* pin, hipStream_t st) const {
    FM_HIP_CHECK(hipMemcpyAsync(dev, pin, bytes, hipMemcpyHostToDevice, st));
    for (int r = 0; r < nruns; ++r)
      if (run_n[r] > 0)
        FM_HIP_CHECK(hipMemcpyAsync(reinterpret_cast<char*>(dev) + o_x + sizeof(float) * run_at[r],
                                    reinterpret_cast<const char*>(pin) + o_x + sizeof(float) * run_at[r],
                                    sizeof(float) * run_n[r], hipMemcpyHostToDevice, st));
  }
};

void check_csr(const fm_csr* c) {
  FM_REQUIRE(c != nullptr, "null fm_csr");
  FM_REQUIRE(c->n_rows >= 0 && c->nnz >= 0, "negative n_rows / nnz");
  FM_REQUIRE(c->n_rows < (int64_t(1) << 31), "n_rows must be < 2^31");
  FM_REQUIRE(c->nnz < (int64_t(1) << 31), "nnz must be < 2^31 per batch");
  FM_REQUIRE(c->n_rows == 0 || (c->row_ptr && c->label), "null row_ptr / label");
  FM_REQUIRE(c->nnz == 0 || (c->col && c->val), "null col / val");
  const int64_t B = c->n_rows;
  if (B > 0) {
    FM_REQUIRE(c->row_ptr[0] == 0, "row_ptr[0] must be 0");
    FM_REQUIRE(c->row_ptr[B] == c->nnz, "row_ptr[n_rows] must equal nnz");
    for (int64_t i = 0; i < B; ++i) FM_REQUIRE(c->row_ptr[i] <= c->row_ptr[i + 1], "row_ptr must be non-decreasing");
  } else {
    FM_REQUIRE(c->nnz == 0, "nnz > 0 with n_rows == 0");
  }
}

static Staged stage_csr(fm_ctx* ctx, const fm_csr* c, bool check_range, Pinned& pin, size_t extra = 0) {
  check_csr(c);
  Staged g;
  const int64_t B = c->n_rows, N = c->nnz;
  g.B = B;
  g.N = N;
  g.o_lab = sizeof(int64_t) * (B + 1);
  g.o_xoff = g.o_lab + sizeof(double) * B;
  g.o_col = (g.o_xoff + sizeof(int32_t) * B + 15) / 16 * 16;
  g.o_x = (g.o_col + sizeof(uint32_t) * N + 15) / 16 * 16;
  g.o_extra = (g.o_x + sizeof(float) * N + 16 + 15) / 16 * 16;  // M <= N
  pin.ensure_slack(g.o_extra + extra);
  const CsrImage im = g.view(pin.p);
  if (B > 0) std::memcpy(im.row_ptr, c->row_ptr, sizeof(int64_t) * (B + 1));
  else im.row_ptr[0] = 0;
  const int64_t F = ctx->cfg.num_features;
  std::atomic<int> bad{0};  // 1 negative id, 2 id >= num_features
  std::atomic<int64_t> mx{-1}, mlen{0};
  // one pass over row chunks: ids (bit 31 = a value follows), labels, the chunk's values packed
  // from its first entry's position on
  std::atomic<int> nrun{0};
  parallel_chunks(B, 4096, [&](int64_t r0, int64_t r1) {
    const int64_t x0 = B > 0 ? c->row_ptr[r0] : 0;
    int64_t lmx = -1, m = x0, llen = 0;
    int lbad = 0;
    for (int64_t i = r0; i < r1; ++i) {
      im.label[i] = c->label[i];  // Double, as the reference's label column (SGD.scala:145-146)
      llen = std::max<int64_t>(llen, c->row_ptr[i + 1] - c->row_ptr[i]);
      im.xoff[i] = (int32_t)m;
      for (int64_t e = c->row_ptr[i]; e < c->row_ptr[i + 1]; ++e) {
        const int32_t id = c->col[e];
        if (id < 0) lbad |= 1;
        else if (check_range && id >= F) lbad |= 2;
        const float x = (float)c->val[e];
        const uint32_t valued = x != 1.0f;
        im.col[e] = (uint32_t)id | (valued << 31);
        im.x[m] = x;  // branch-free: the slot is taken only by a value that is not 1
        m += valued;
        lmx = std::max<int64_t>(lmx, id);
      }
    }
    const int ri = nrun.fetch_add(1);
    g.run_at[ri] = x0;
    g.run_n[ri] = m - x0;
    if (lbad) bad.fetch_or(lbad);
    int64_t cur = mx.load();
    while (lmx > cur && !mx.compare_exchange_weak(cur, lmx)) {
    }
    cur = mlen.load();
    while (llen > cur && !mlen.compare_exchange_weak(cur, llen)) {
    }
  });
  FM_REQUIRE(!(bad.load() & 1), "negative feature id");
  FM_REQUIRE(!(bad.load() & 2), "feature id >= num_features");
  g.nruns = nrun.load();
  for (int r = 0; r < g.nruns; ++r) g.M += g.run_n[r];
  g.bytes = g.o_col + sizeof(uint32_t) * N;
  g.max_id = mx.load();
  g.max_len = mlen.load();
  return g;
}

// The fused step (fm_device.h "Singleton rows") for batches this context prepares: a
// single-table context with kp <= 16; by default (FM_FUSE_DEFAULT) only for a table larger than
// the 256-MB Infinity Cache, where the update's re-read of the singleton rows goes to HBM -- a
// cache-resident table re-reads them on-die, and the split and tags would cost more than they save
// (c2 / c5: 0.245 / 0.273 ms per step fused against 0.184 / 0.208 unfused, profiles/r03_v1).
bool fuse_rule(const fm_ctx* ctx) {
  // the fused forward applies the singleton rows with the squared residual, before the objective stage
  // (fm_objective.hip) has replaced it: another loss never fuses
  if (ctx->cfg.loss != FM_LOSS_SQUARED) return false;
  if (ctx->cfg.fuse_single == FM_FUSE_OFF || ctx->kp > 16) return false;
  const double table_bytes = (double)ctx->rows * ctx->stride * sizeof(float);
  return ctx->cfg.fuse_single == FM_FUSE_ON || table_bytes > 256.0 * 1024 * 1024;
}

static const char* loss_name(int32_t loss) {
  return loss == FM_LOSS_LOGISTIC ? "FM_LOSS_LOGISTIC" : loss == FM_LOSS_BPR ? "FM_LOSS_BPR" : "FM_LOSS_SQUARED";
}

void require_squared(const fm_ctx* ctx, const char* call) {
  FM_REQUIRE(ctx->cfg.loss == FM_LOSS_SQUARED, std::string(call) + " runs the squared step only: this context's loss is " +
                                                   loss_name(ctx->cfg.loss));
}

static bool fuse_on(const fm_ctx* ctx) { return ctx->cfg.shard_count == 1 && fuse_rule(ctx); }

static bool batch_fits(const fm_batch* b, const Staged& g) {
  const BatchBytes z = batch_bytes(g.B, g.N);
  return b->dev.row_ptr.bytes >= z.row_ptr && b->dev.col.bytes >= z.col && b->dev.ent.bytes >= z.ent &&
         b->dev.xs.bytes >= z.xs && b->dev.label.bytes >= z.label && b->up.bytes >= g.o_x + sizeof(float) * g.N + 16;
}

// b's device buffers (grown, never shrunk) filled from the staging by the image's async copies on st
// (into b->up, the staging's device image), then col / label / row_ptr and the exploded entries are
// laid out from it by one kernel pass on st.
static void copy_staged(fm_ctx* ctx, const Staged& g, const Pinned& pin, fm_batch* b, hipStream_t st) {
  b->owner = ctx;
  b->device = ctx->cfg.device;
  b->max_id = g.max_id;
  size_batch(b->dev, g.B, g.N);
  b->up.ensure_slack(g.o_x + sizeof(float) * g.N + 16);
  g.enqueue_copies(b->up.p, pin.p, st);
  launch_explode(g.view(b->up.p), g.B, g.N, b->dev, st);
}

// Synchronous upload (fm_batch_create, fm_predict, fm_loss_grad): staged in the context's
// pinned buffer, copied on the context's stream, returns after the copies.
void upload_batch(fm_ctx* ctx, const fm_csr* c, fm_batch* b, bool check_range) {
  FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the staging / b may still feed queued work
  const Staged g = stage_csr(ctx, c, check_range, ctx->up_pin);
  copy_staged(ctx, g, ctx->up_pin, b, ctx->stream);
  FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
}

// The context's reusable batch for the synchronous host-buffer entry points (fm_predict,
// fm_loss_grad): its device buffers persist across calls.
fm_batch* host_batch(fm_ctx* ctx) {
  if (!ctx->host_batch) ctx->host_batch.reset(new fm_batch());
  return ctx->host_batch.get();
}

OutBatch out_batch(fm_ctx* ctx, const fm_batch* data, fm_batch** out, bool group) {
  OutBatch o;
  o.out = out;
  o.b = *out;
  if (o.b == nullptr) {
    o.fresh.reset(group ? new_group_batch(ctx) : new fm_batch());
    o.b = o.fresh.get();
    o.b->owner = ctx;
    o.b->device = ctx->cfg.device;
  } else {
    FM_REQUIRE(o.b->owner == ctx && o.b != data && !o.b->grp == !group && o.b->split_rows.empty(),
               "out must be a batch of this context other than data");
  }
  return o;
}

// A batch refilled by fm_batch_from_rows is written on the side stream: a reader on stream st waits
// for that (a no-op for batches that were never refilled).
void wait_built(const fm_batch* b, hipStream_t st) {
  if (b->built) FM_HIP_CHECK(hipStreamWaitEvent(st, b->built, 0));
}

double* eval_next_slot(fm_ctx* ctx) {
  ctx->ensure_eval_hist(ctx->eval_n + 1);
  return ctx->eval_hist.as<double>() + kEvalRec * ctx->eval_n;
}

void eval_read(const double* rec, int64_t epoch, fm_eval_out* out) {
  out->n_rows = (int64_t)rec[0];
  out->n_unlearned = (int64_t)rec[1];
  out->epoch = epoch;
  out->sum_err = rec[2];
  out->sum_abs_err = rec[3];
  out->sum_sq_err = rec[4];
}

void eval_commit(fm_ctx* ctx, fm_eval_out* out) {
  const double* slot = ctx->eval_hist.as<double>() + kEvalRec * ctx->eval_n;
  ctx->eval_epoch.push_back(ctx->epoch);
  ctx->eval_n += 1;
  if (!out) return;
  ctx->pinned.ensure(64);
  FM_HIP_CHECK(hipMemcpyAsync(ctx->pinned.p, slot, sizeof(double) * kEvalRec, hipMemcpyDeviceToHost, ctx->stream));
  FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  eval_read(reinterpret_cast<const double*>(ctx->pinned.p), ctx->epoch, out);
}

void reserve_work(fm_ctx* ctx, int64_t B, int64_t N) {
  StepWork& w = ctx->work;
  w.S.ensure_slack(sizeof(float) * (size_t)std::max<int64_t>(B, 1) * s_rec_floats(ctx->kp));
  w.yl.ensure_slack(sizeof(float2) * (size_t)std::max<int64_t>(B, 1));
  w.sort.ensure(std::max<int64_t>(N, 1));
  const int64_t nranges = (N + 255) / 256;  // update waves (fm_update.hip, kWaveEnt)
  w.part.ensure_slack(sizeof(double) * (size_t)std::max<int64_t>(nranges, 1) * 2 * (ctx->kp + 2));
  w.ucnt.ensure_slack(sizeof(uint32_t) * (size_t)std::max<int64_t>((N + 1023) / 1024, 1));
  w.loss_part.ensure(sizeof(double2) * kLossPartBlocks);
}

}  // namespace fmhip

namespace {

// One fused step.  emit != nullptr (replicated mode, fm_repl_grad): the per-slot gradient sums
// are written to emit[rows][kp + 4] instead of being applied, and the epoch does not advance.
int step_impl(fm_ctx* ctx, fm_batch* b, int32_t t, double step_size, double reg_param, fm_step_out* out,
              float* emit = nullptr) {
  FM_REQUIRE(b != nullptr, "null batch");
  FM_REQUIRE(b->owner == ctx, "batch belongs to another context");
  FM_REQUIRE(ctx->cfg.shard_count == 1, "sharded contexts step through the fm_shard_* entry points");
  FM_REQUIRE(b->split_rows.empty(), "a dataset made by fm_batch_create_splits is stepped through its split views");
  const int32_t loss = ctx->cfg.loss;
  FM_REQUIRE(loss != FM_LOSS_BPR || (b->row_group >= 2 && b->dev.n_rows % b->row_group == 0),
             "an FM_LOSS_BPR step needs a grouped batch: fm_batch_sample_pairs with n_neg >= 1, or fm_batch_set_group");
  if (emit) FM_HIP_CHECK(hipMemsetAsync(emit, 0, sizeof(float) * (size_t)ctx->rows * (ctx->kp + 4), ctx->stream));
  if (b->dev.n_rows == 0) return FM_NOTHING_TO_DO;  // SGD.scala:126-128
  FM_REQUIRE(t >= 1, "iteration index t must be >= 1");
  FM_REQUIRE(std::isfinite(step_size) && std::isfinite(reg_param), "non-finite step size / regParam");
  const int64_t B = b->dev.n_rows, N = b->dev.nnz;
  reserve_work(ctx, B, N);
  ctx->ensure_hist(ctx->epoch + 1);
  StepParams p;
  p.n_rows = B;
  p.eta = step_size / std::sqrt((double)t);  // SGD.scala:121
  p.lam = p.eta * reg_param;                 // SGD.scala:122
  p.m = (double)B;                           // miniBatchSize, SGD.scala:124
  p.scale_v = p.eta / (double)B;             // currentStepSize / miniBatchSize, SGD.scala:153
  p.epoch = ctx->epoch;
  p.cumE = ctx->cum_host.back();
  p.cum_next = p.cumE + p.lam;
  p.w0 = ctx->cfg.w0;
  const TableView T = ctx->view();
  wait_built(b, ctx->stream);
  int64_t nfwd = 0;
  const uint32_t* skeys = nullptr;
  const uint2* sents = nullptr;
  const bool prepared = b->prepared;
  const bool fused = prepared && b->split;  // the view holds the multi runs only (fm_batch_prepare)
  FM_REQUIRE(!(fused && emit), "a batch prepared for the fused step cannot feed fm_repl_grad");
  FM_REQUIRE(ctx->epoch < (1 << 29), "epoch count beyond the multi tags' range (2^29 steps)");
  if (prepared) {
    // sorted ahead of time by fm_batch_prepare on the side stream
    skeys = b->skeys.as<uint32_t>();
    sents = b->sents.as<uint2>();
  } else {
    // fork: the sort only reads the batch, so it runs on the side stream beside the forward
    FM_HIP_CHECK(hipEventRecord(ctx->ev_fork, ctx->stream));
    FM_HIP_CHECK(hipStreamWaitEvent(ctx->side, ctx->ev_fork, 0));
    hipEvent_t es = ctx->prof_begin(ctx->side);
    radix_sort_pairs64(ctx->work.sort, b->dev.col.as<uint32_t>(), b->dev.ent.as<uint2>(), N, bits_for(ctx->rows - 1),
                       ctx->side, &skeys, &sents);
    ctx->prof_end("sort", es, ctx->side);
    FM_HIP_CHECK(hipEventRecord(ctx->ev_join, ctx->side));
  }
  hipEvent_t e0 = nullptr;
  FwdOut fx{};
  if (fused) {
    // the batch's sorted view (fm_batch_prepare, a step ahead on the side stream) split here, on the
    // main stream: its runs of two or more entries into the multi view, each multi run's row tagged
    // with this step's epoch by the count pass as it finds the run (the split on the side stream with a
    // separate tag pass at the step measured 0.968-0.971 against 0.924-0.931 ms per c3 step, three
    // alternating reps, profiles/r04_i)
    FM_HIP_CHECK(hipStreamWaitEvent(ctx->stream, b->ready, 0));
    e0 = ctx->prof_begin(ctx->stream);
    launch_split(b->fkeys.as<uint32_t>(), b->fents.as<uint2>(), N, ctx->split_work, b->skeys.as<uint32_t>(),
                 b->sents.as<uint2>(), b->split_n.as<int64_t>(), ctx->stream, T, p.epoch);
    ctx->prof_end("split", e0, ctx->stream);
    fx.mode = kTrainFused;
  }
  e0 = ctx->prof_begin(ctx->stream);
  launch_forward(T, b->dev, ctx->work, p, ctx->stream, &nfwd, nullptr, fused ? &fx : nullptr);
  ctx->prof_end("forward", e0, ctx->stream);
  if (loss != FM_LOSS_SQUARED) {
    // the objective stage: {r, yhat} -> {r, r} with the loss's own r, and its loss partials in place of
    // the forward's (a squared context launches nothing here)
    FM_REQUIRE(!fused && !emit, "the fused and the replicated step are the squared loss's");
    e0 = ctx->prof_begin(ctx->stream);
    nfwd = launch_objective(loss, b->row_group, ctx->kp, b->dev, ctx->work, ctx->stream);
    ctx->prof_end("objective", e0, ctx->stream);
  }
  // (the prepared batch's wait moved before the forward, where its sort has long finished, measured
  // 0.170-0.173 against 0.167-0.168 ms at c2 and 0.191-0.192 against 0.187-0.190 at c5, three
  // alternating reps, profiles/r05_h/ab: not taken)
  if (!fused) FM_HIP_CHECK(hipStreamWaitEvent(ctx->stream, prepared ? b->ready : ctx->ev_join, 0));
  e0 = ctx->prof_begin(ctx->stream);
  double* stats = ctx->loss_hist.as<double>() + 3 * (int64_t)ctx->epoch;
  launch_segment_update(T, b->dev, ctx->work, p, skeys, sents, nfwd, stats, ctx->stream, emit,
                        fused ? b->split_n.as<int64_t>() : nullptr);
  // the shared sort workspace is read by the main stream only when the batch was sorted inline
  // (not prepared): only then must the next fm_batch_prepare's sort wait for this update
  if (!prepared) FM_HIP_CHECK(hipEventRecord(ctx->ev_upd_done, ctx->stream));
  // the last read of the batch (its next fm_batch_prepare or fm_batch_from_rows refill waits for it)
  if (b->last_use) FM_HIP_CHECK(hipEventRecord(b->last_use, ctx->stream));
  b->prepared = false;
  ctx->prof_end("update", e0, ctx->stream);
  if (emit) return FM_OK;
  ctx->epoch += 1;
  ctx->cum_host.push_back(p.cum_next);
  if (out) {
    ctx->pinned.ensure(64);
    FM_HIP_CHECK(hipMemcpyAsync(ctx->pinned.p, stats, sizeof(double) * 3, hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const double* h = reinterpret_cast<const double*>(ctx->pinned.p);
    out->loss_sum = h[0];
    out->n_loss_rows = (int64_t)h[1];
    out->n_unique = (int64_t)h[2];
    out->n_rows = B;
  }
  return FM_OK;
}

}  // namespace

extern "C" {

const char* fm_last_error(void) { return g_last_error.c_str(); }

int64_t fm_device_bytes_live(void) { return g_dev_bytes_live.load(std::memory_order_relaxed); }
int64_t fm_device_allocs_live(void) { return g_dev_allocs_live.load(std::memory_order_relaxed); }

int fm_create(const fm_config* cfg, fm_ctx** out) {
  return guarded_free([&]() -> int {
    FM_REQUIRE(cfg && out, "null argument");
    FM_REQUIRE(cfg->loss == FM_LOSS_SQUARED || cfg->loss == FM_LOSS_LOGISTIC || cfg->loss == FM_LOSS_BPR,
               "loss must be FM_LOSS_SQUARED, FM_LOSS_LOGISTIC or FM_LOSS_BPR");
    if (cfg->loss != FM_LOSS_SQUARED) {
      const std::string nm = loss_name(cfg->loss);
      FM_REQUIRE(cfg->parallel == FM_PARALLEL_NONE,
                 "loss = " + nm + " needs parallel == FM_PARALLEL_NONE: multi-GPU objectives are not built yet");
      FM_REQUIRE(cfg->shard_count == 1, "loss = " + nm + " needs shard_count == 1: multi-GPU objectives are not built yet");
      FM_REQUIRE(cfg->fuse_single != FM_FUSE_ON,
                 "loss = " + nm + " cannot take fuse_single = FM_FUSE_ON: the fused forward applies singleton rows with the "
                 "squared residual");
    }
    FM_REQUIRE(cfg->wire == FM_WIRE_FP32 || cfg->wire == FM_WIRE_FP64, "wire must be FM_WIRE_FP32 or FM_WIRE_FP64");
    FM_REQUIRE(cfg->wire != FM_WIRE_FP64 || cfg->parallel != FM_PARALLEL_REPLICATED,
               "wire = FM_WIRE_FP64 applies to the sharded step only: the replicated gradient all-reduce is fp32");
    if (cfg->parallel != FM_PARALLEL_NONE) return group_create(cfg, out);  // several ranks (fm_group.hip)
    FM_REQUIRE(cfg->num_features >= 1 && cfg->num_features <= (int64_t(1) << 31), "num_features must be in [1, 2^31]");
    FM_REQUIRE(cfg->k >= 1 && cfg->k <= 256, "dimFactorization must be in [1, 256]");
    FM_REQUIRE(cfg->shard_count >= 1 && cfg->shard_index >= 0 && cfg->shard_index < cfg->shard_count,
               "bad shard_index / shard_count");
    FM_REQUIRE(cfg->init_sd >= 0.0, "init_sd must be >= 0");
    FM_REQUIRE(cfg->fuse_single == FM_FUSE_DEFAULT || cfg->fuse_single == FM_FUSE_ON || cfg->fuse_single == FM_FUSE_OFF,
               "fuse_single must be FM_FUSE_DEFAULT, FM_FUSE_ON or FM_FUSE_OFF");
    int ndev = 0;
    FM_HIP_CHECK(hipGetDeviceCount(&ndev));
    FM_REQUIRE(cfg->device >= 0 && cfg->device < ndev, "device ordinal out of range");
    FM_HIP_CHECK(hipSetDevice(cfg->device));
    std::unique_ptr<fm_ctx> c(new fm_ctx());
    c->cfg = *cfg;
    c->kp = (cfg->k + 3) / 4 * 4;
    c->rows = (cfg->num_features - cfg->shard_index + cfg->shard_count - 1) / cfg->shard_count;
    // (the step's stream at high priority and the side stream at the lowest measured slower: c3
    // 0.984-0.996 against 0.946-0.951 ms)
    FM_HIP_CHECK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
    FM_HIP_CHECK(hipStreamCreateWithFlags(&c->side_own, hipStreamNonBlocking));
    c->side = c->side_own;
    FM_HIP_CHECK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
    FM_HIP_CHECK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
    FM_HIP_CHECK(hipEventCreateWithFlags(&c->ev_upd_done, hipEventDisableTiming));
    FM_HIP_CHECK(hipEventRecord(c->ev_upd_done, c->stream));
    c->stride = record_stride(c->kp);
    c->rec.ensure(sizeof(float) * (size_t)std::max<int64_t>(c->rows, 1) * c->stride);
    c->ensure_hist(4096);
    launch_table_reset(c->view(), c->stream);
    FM_HIP_CHECK(hipStreamSynchronize(c->stream));
    *out = c.release();
    return FM_OK;
  });
}

void fm_destroy(fm_ctx* ctx) {
  if (!ctx) return;
  try {
    delete ctx;
  } catch (...) {
  }
}

int fm_set_stream(fm_ctx* ctx, void* s) {
  if (ctx && ctx->group) {  // a multi-GPU context: only with one local rank, whose streams these become
    if (ctx->cfg.n_gpus != 1) {
      set_error("fm_set_stream on a context with several local ranks");
      return FM_ERR_ARG;
    }
    return fm_set_stream(group_member0(ctx), s);
  }
  return guarded(ctx, [&]() -> int {
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream && ctx->stream) FM_HIP_CHECK(hipStreamDestroy(ctx->stream));
    // NULL selects the device's default (null) stream, which is what torch's default stream is
    ctx->stream = reinterpret_cast<hipStream_t>(s);
    ctx->own_stream = false;
    return FM_OK;
  });
}

int fm_set_side_stream(fm_ctx* ctx, void* s) {
  if (ctx && ctx->group) {  // a multi-GPU context: only with one local rank, whose streams these become
    if (ctx->cfg.n_gpus != 1) {
      set_error("fm_set_side_stream on a context with several local ranks");
      return FM_ERR_ARG;
    }
    return fm_set_side_stream(group_member0(ctx), s);
  }
  return guarded(ctx, [&]() -> int {
    FM_HIP_CHECK(hipStreamSynchronize(ctx->side));
    ctx->side = s ? reinterpret_cast<hipStream_t>(s) : ctx->side_own;
    return FM_OK;
  });
}

int fm_sync(fm_ctx* ctx) {
  return guarded(ctx, [&]() -> int {
    if (ctx->group) return group_sync(ctx);
    // every stream the context enqueues on: the step's, the side stream's preparations and the copy
    // stream's fm_batch_from_rows gathers (after this the caller may free a dataset it gathered from)
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->side));
    if (ctx->copy_stream) FM_HIP_CHECK(hipStreamSynchronize(ctx->copy_stream));
    return FM_OK;
  });
}

int fm_reserve(fm_ctx* ctx, int64_t max_rows, int64_t max_nnz) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(max_rows >= 0 && max_nnz >= 0, "negative reserve");
    if (ctx->group) return group_reserve(ctx, max_rows, max_nnz);
    reserve_work(ctx, max_rows, max_nnz);
    return FM_OK;
  });
}

int fm_load_tables(fm_ctx* ctx, const int32_t* ids, int64_t n, const double* w, const double* V) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(n >= 0, "negative n");
    if (n == 0) return FM_OK;
    if (ctx->group) return group_load_tables(ctx, ids, n, w, V);
    FM_REQUIRE(ids && w && V, "null argument");
    for (int64_t i = 0; i < n; ++i)
      FM_REQUIRE(ids[i] >= 0 && ids[i] < ctx->cfg.num_features, "id out of [0, num_features)");
    DevBuf di, dw, dv;
    di.ensure(sizeof(int32_t) * n);
    dw.ensure(sizeof(double) * n);
    dv.ensure(sizeof(double) * n * ctx->cfg.k);
    FM_HIP_CHECK(hipMemcpy(di.p, ids, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    FM_HIP_CHECK(hipMemcpy(dw.p, w, sizeof(double) * n, hipMemcpyHostToDevice));
    FM_HIP_CHECK(hipMemcpy(dv.p, V, sizeof(double) * n * ctx->cfg.k, hipMemcpyHostToDevice));
    launch_load_rows(ctx->view(), di.as<int32_t>(), n, dw.as<double>(), dv.as<double>(), ctx->epoch,
                     ctx->cum_host.back(), ctx->stream);
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return FM_OK;
  });
}

int fm_init_random(fm_ctx* ctx, const int32_t* ids, int64_t n) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(n >= 0, "negative n");
    if (n == 0) return FM_OK;
    FM_REQUIRE(ids, "null ids");
    if (ctx->group) return group_init_random(ctx, ids, n, 0, 0);
    for (int64_t i = 0; i < n; ++i)
      FM_REQUIRE(ids[i] >= 0 && ids[i] < ctx->cfg.num_features, "id out of [0, num_features)");
    DevBuf di;
    di.ensure(sizeof(int32_t) * n);
    FM_HIP_CHECK(hipMemcpy(di.p, ids, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    launch_init_random(ctx->view(), di.as<int32_t>(), n, 0, ctx->cfg.seed, ctx->cfg.init_sd, ctx->epoch,
                       ctx->cum_host.back(), ctx->stream);
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return FM_OK;
  });
}

int fm_init_random_range(fm_ctx* ctx, int64_t b, int64_t e) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(b >= 0 && e >= b && e <= ctx->cfg.num_features, "bad id range");
    if (ctx->group) return group_init_random(ctx, nullptr, 0, b, e);
    launch_init_random(ctx->view(), nullptr, e - b, b, ctx->cfg.seed, ctx->cfg.init_sd, ctx->epoch,
                       ctx->cum_host.back(), ctx->stream);
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return FM_OK;
  });
}

int64_t fm_num_present(fm_ctx* ctx) {
  int64_t n = -1;
  int rc = guarded(ctx, [&]() -> int {
    if (ctx->group) {
      n = group_num_present(ctx);
      return FM_OK;
    }
    DevBuf d;
    d.ensure(sizeof(int64_t));
    launch_count_present(ctx->view(), d.as<int64_t>(), ctx->stream);
    FM_HIP_CHECK(hipMemcpyAsync(&n, d.p, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return FM_OK;
  });
  return rc == FM_OK ? n : rc;
}

int64_t fm_epoch(fm_ctx* ctx) { return ctx ? ctx->epoch : -1; }

int fm_export_tables(fm_ctx* ctx, int32_t* ids, double* w, double* V, int64_t cap, int64_t* n) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(n != nullptr && cap >= 0, "bad arguments");
    if (ctx->group) return group_export_tables(ctx, ids, w, V, cap, n);
    launch_flush(ctx->view(), ctx->epoch, ctx->cum_host.back(), ctx->stream);  // apply pending L1 to every row
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    const int k = ctx->cfg.k, kp = ctx->kp, S = ctx->stride;
    const int64_t chunk_rows = std::max<int64_t>(1, (int64_t(64) << 20) / (4 * S));
    std::vector<float> hv;
    int64_t cnt = 0, o = 0;
    const bool fill = cap > 0;
    for (int64_t r0 = 0; r0 < ctx->rows; r0 += chunk_rows) {
      const int64_t r1 = std::min(ctx->rows, r0 + chunk_rows);
      hv.resize((size_t)(r1 - r0) * S);
      FM_HIP_CHECK(hipMemcpy(hv.data(), ctx->rec.as<float>() + r0 * S, sizeof(float) * (r1 - r0) * S,
                             hipMemcpyDeviceToHost));
      for (int64_t i = r0; i < r1; ++i) {
        const float* row = hv.data() + (size_t)(i - r0) * S;
        RowHdr hd;
        std::memcpy(&hd, row + kp, sizeof(RowHdr));
        if (hd.t < 0) continue;
        ++cnt;
        if (!fill) continue;
        FM_REQUIRE(o < cap && ids && w && V, "export buffers too small or null");
        ids[o] = (int32_t)(i * ctx->cfg.shard_count + ctx->cfg.shard_index);
        w[o] = hd.w;
        for (int f = 0; f < k; ++f) V[o * k + f] = row[f];
        ++o;
      }
    }
    *n = cnt;
    return FM_OK;
  });
}

int fm_export_rows(fm_ctx* ctx, const int32_t* ids, int64_t n, double* w, double* V, int8_t* present) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(n >= 0, "negative n");
    if (n == 0) return FM_OK;
    FM_REQUIRE(ids && w && V && present, "null argument");
    if (ctx->group) return group_export_rows(ctx, ids, n, w, V, present);
    const int R = ctx->cfg.shard_count;
    for (int64_t i = 0; i < n; ++i) {
      FM_REQUIRE(ids[i] >= 0 && ids[i] < ctx->cfg.num_features, "id out of [0, num_features)");
      FM_REQUIRE(ids[i] % R == ctx->cfg.shard_index, "id not owned by this shard");
    }
    const int k = ctx->cfg.k;
    DevBuf di, dw, dv, dp;
    di.ensure(sizeof(int32_t) * n);
    dw.ensure(sizeof(double) * n);
    dv.ensure(sizeof(double) * n * k);
    dp.ensure(sizeof(int8_t) * n);
    FM_HIP_CHECK(hipMemcpyAsync(di.p, ids, sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx->stream));
    launch_gather_rows(ctx->view(), di.as<int32_t>(), n, ctx->cum_host.back(), dw.as<double>(), dv.as<double>(),
                       dp.as<int8_t>(), ctx->stream);
    FM_HIP_CHECK(hipMemcpyAsync(w, dw.p, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipMemcpyAsync(V, dv.p, sizeof(double) * n * k, hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipMemcpyAsync(present, dp.p, sizeof(int8_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return FM_OK;
  });
}

int fm_batch_create(fm_ctx* ctx, const fm_csr* csr, fm_batch** out) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(out != nullptr, "null out");
    if (ctx->group) return group_batch_create(ctx, csr, out);
    std::unique_ptr<fm_batch> b(new fm_batch());
    upload_batch(ctx, csr, b.get(), true);
    // kept for fm_batch_from_rows (a cached dataset's splits sized on the host)
    b->host_rp.assign(csr->row_ptr, csr->row_ptr + csr->n_rows + 1);
    *out = b.release();
    return FM_OK;
  });
}

void fm_batch_destroy(fm_batch* b) {
  if (!b) return;
  try {
    delete b;
  } catch (...) {
  }
}

int fm_batch_prepare(fm_ctx* ctx, fm_batch* b) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(b != nullptr && b->owner == ctx, "batch belongs to another context");
    if (ctx->group) return group_batch_prepare(ctx, b);
    FM_REQUIRE(ctx->cfg.shard_count == 1, "fm_batch_prepare is for single-table contexts");
    FM_REQUIRE(b->split_rows.empty(), "a dataset made by fm_batch_create_splits is prepared through its split views");
    const int64_t N = b->dev.nnz;
    if (N == 0) return FM_OK;
    b->ensure_events(ctx->stream);
    b->skeys.ensure_slack(sizeof(uint32_t) * N);
    b->sents.ensure_slack(sizeof(uint2) * N);
    // the shared sort workspace and this batch's view may still be read by an enqueued step; a batch
    // refilled by fm_batch_from_rows is sorted once its gather is done
    FM_HIP_CHECK(hipStreamWaitEvent(ctx->side, ctx->ev_upd_done, 0));
    FM_HIP_CHECK(hipStreamWaitEvent(ctx->side, b->last_use, 0));
    wait_built(b, ctx->side);
    hipEvent_t es = ctx->prof_begin(ctx->side);
    const uint32_t* sk = nullptr;
    const uint2* sv = nullptr;
    b->split = fuse_on(ctx);
    const int kb = bits_for(ctx->rows - 1);
    const uint32_t* col = b->dev.col.as<uint32_t>();
    const uint2* ent = b->dev.ent.as<uint2>();
    if (b->split) {
      // the fused step's batch: the whole sorted view (fkeys / fents), which the step splits into the
      // multi view (skeys / sents, {their count, the number of singleton runs} in split_n)
      b->split_n.ensure(2 * sizeof(int64_t));
      b->fkeys.ensure_slack(sizeof(uint32_t) * N);
      b->fents.ensure_slack(sizeof(uint2) * N);
      radix_sort_pairs64(ctx->work.sort, col, ent, N, kb, ctx->side, &sk, &sv, b->fkeys.as<uint32_t>(),
                         b->fents.as<uint2>());
    } else {
      radix_sort_pairs64(ctx->work.sort, col, ent, N, kb, ctx->side, &sk, &sv, b->skeys.as<uint32_t>(),
                         b->sents.as<uint2>());
    }
    ctx->prof_end("sort", es, ctx->side);
    FM_HIP_CHECK(hipEventRecord(b->ready, ctx->side));
    b->prepared = true;
    return FM_OK;
  });
}

int fm_batch_from_rows(fm_ctx* ctx, const fm_batch* data, const int64_t* rows, int64_t n, fm_batch** out) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(out != nullptr && data != nullptr, "null argument");
    FM_REQUIRE(data->owner == ctx, "data belongs to another context");
    FM_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "n out of range");
    FM_REQUIRE(n == 0 || rows != nullptr, "null rows");
    if (ctx->group) return group_batch_from_rows(ctx, data, rows, n, out);
    const int64_t Bd = data->dev.n_rows;
    FM_REQUIRE((int64_t)data->host_rp.size() == Bd + 1,
               "data must be a batch made by fm_batch_create");
    OutBatch res = out_batch(ctx, data, out, false);
    fm_batch* b = res.b;
    // a split view refilled as a selection: its borrowed pointers are dropped, its own buffers grown below
    b->detach_view();
    b->ensure_events(ctx->stream);
    // the staging {rows, row_ptr} of this batch's previous selection has been copied out (a batch never
    // refilled before has no staging in flight: its events are made and nothing is waited for, so the
    // first refill returns once it is enqueued whatever the streams hold)
    if (!b->built) {
      FM_HIP_CHECK(hipEventCreateWithFlags(&b->built, hipEventDisableTiming));
      FM_HIP_CHECK(hipEventCreateWithFlags(&b->sel_copied, hipEventDisableTiming));
    } else {
      FM_HIP_CHECK(hipEventSynchronize(b->sel_copied));
    }
    const size_t img = sizeof(int64_t) * (2 * (size_t)n + 1);
    b->sel_pin.ensure_slack(img);
    int64_t* hrows = reinterpret_cast<int64_t*>(b->sel_pin.p);
    int64_t* rp = hrows + n;
    // the rows and their result row_ptr straight into the pinned staging, from the dataset's row_ptr
    // (validated on the way)
    FM_REQUIRE(selection_row_ptr(data->host_rp.data(), Bd, rows, n, hrows, rp), "row index out of [0, rows of data)");
    const int64_t N = rp[n];
    FM_REQUIRE(N < (int64_t(1) << 31), "nnz must be < 2^31 per batch");
    // batch-only work on the copy stream, behind every queued step that reads this batch: the copy
    // of the next split overlaps the sort of the current one on the side stream (the sort waits
    // for `built`, fm_batch_prepare)
    if (!ctx->copy_stream) FM_HIP_CHECK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    hipStream_t gs = ctx->copy_stream;
    // the refill rewrites what queued work may still read: the last step of the batch (b->last_use,
    // recorded by the single-table step and by the sharded owner update on the main stream), the
    // sharded iteration's own last read (sh->last_use) and a preparation never stepped (its sort on the
    // side stream reads dev.col / dev.ent)
    FM_HIP_CHECK(hipStreamWaitEvent(gs, b->last_use, 0));
    if (b->sh && b->sh->last_use) FM_HIP_CHECK(hipStreamWaitEvent(gs, b->sh->last_use, 0));
    if (b->prepared && b->ready) FM_HIP_CHECK(hipStreamWaitEvent(gs, b->ready, 0));
    b->max_id = data->max_id;
    size_batch(b->dev, n, N);
    b->up.ensure_slack(img + 16);
    FM_HIP_CHECK(hipMemcpyAsync(b->up.p, b->sel_pin.p, img, hipMemcpyHostToDevice, gs));
    FM_HIP_CHECK(hipEventRecord(b->sel_copied, gs));
    if (n > 0) {
      const int64_t* up = b->up.as<int64_t>();
      launch_select_rows(data->dev, up, up + n, n, b->dev, gs);
    } else {
      FM_HIP_CHECK(hipMemcpyAsync(b->dev.row_ptr.p, b->up.as<int64_t>(), sizeof(int64_t), hipMemcpyDeviceToDevice, gs));
    }
    FM_HIP_CHECK(hipEventRecord(b->built, gs));
    b->prepared = false;  // a refilled batch is sorted again by its own fm_batch_prepare
    b->host_rp.clear();   // a selection is not itself a dataset (fm_batch_create's batches are)
    b->row_group = 0;
    res.commit();
    return FM_OK;
  });
}

int fm_batch_create_splits(fm_ctx* ctx, const fm_csr* csr, int32_t n_splits, const int64_t* split_rows,
                           fm_batch** out) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(out != nullptr && csr != nullptr, "null argument");
    FM_REQUIRE(n_splits >= 1 && split_rows != nullptr, "n_splits must be >= 1");
    FM_REQUIRE(split_rows[0] == 0 && split_rows[n_splits] == csr->n_rows, "split_rows must run from 0 to n_rows");
    for (int32_t i = 0; i < n_splits; ++i) FM_REQUIRE(split_rows[i] <= split_rows[i + 1], "split_rows must be non-decreasing");
    if (ctx->group) return group_batch_create_splits(ctx, csr, n_splits, split_rows, out);
    std::unique_ptr<fm_batch> b(new fm_batch());
    upload_batch(ctx, csr, b.get(), true);
    b->host_rp.assign(csr->row_ptr, csr->row_ptr + csr->n_rows + 1);
    b->split_rows.assign(split_rows, split_rows + n_splits + 1);
    DevBuf dsr;
    dsr.ensure(sizeof(int64_t) * (n_splits + 1));
    FM_HIP_CHECK(hipMemcpyAsync(dsr.p, split_rows, sizeof(int64_t) * (n_splits + 1), hipMemcpyHostToDevice, ctx->stream));
    b->split_rp.ensure(sizeof(int64_t) * (csr->n_rows + n_splits));
    launch_split_rebase(b->dev, dsr.as<int64_t>(), n_splits, b->split_rp.as<int64_t>(), ctx->stream);
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *out = b.release();
    return FM_OK;
  });
}

int fm_batch_layout_splits(fm_ctx* ctx, const fm_csr* csr, int32_t n_splits, const int64_t* split_rows,
                           const int64_t* order, fm_batch** out) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(out != nullptr && csr != nullptr, "null argument");
    FM_REQUIRE(n_splits >= 1 && split_rows != nullptr, "n_splits must be >= 1");
    FM_REQUIRE(split_rows[0] == 0, "split_rows must start at 0");
    for (int32_t i = 0; i < n_splits; ++i) FM_REQUIRE(split_rows[i] <= split_rows[i + 1], "split_rows must be non-decreasing");
    const int64_t n = split_rows[n_splits];  // laid-out rows
    FM_REQUIRE(n < (int64_t(1) << 31), "laid-out rows must be < 2^31");
    FM_REQUIRE(n == 0 || order != nullptr, "null order");
    if (ctx->group) return group_batch_layout_splits(ctx, csr, n_splits, split_rows, order, out);
    std::unique_ptr<fm_batch> b(new fm_batch());
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));  // the staging may still feed queued work
    // the source in its own row order, staged as any upload (validated on the way), and behind it
    // {order [n], the laid-out row_ptr [n + 1], split_rows [n_splits + 1]}
    const size_t extra = sizeof(int64_t) * (2 * (size_t)n + 1 + (size_t)n_splits + 1);
    const Staged g = stage_csr(ctx, csr, true, ctx->up_pin, extra);
    const int64_t D = g.B;
    int64_t* hord = reinterpret_cast<int64_t*>(reinterpret_cast<char*>(ctx->up_pin.p) + g.o_extra);
    int64_t* rp = hord + n;
    int64_t* hsr = rp + n + 1;
    FM_REQUIRE(selection_row_ptr(csr->row_ptr, D, order, n, hord, rp), "row index out of [0, n_rows of csr)");
    const int64_t N = rp[n];  // laid-out entries
    FM_REQUIRE(N < (int64_t(1) << 31), "nnz must be < 2^31 per batch");
    std::copy(split_rows, split_rows + n_splits + 1, hsr);
    hipStream_t st = ctx->stream;
    b->owner = ctx;
    b->device = ctx->cfg.device;
    b->max_id = g.max_id;
    size_batch(b->dev, n, N);
    b->split_rp.ensure(sizeof(int64_t) * (n + n_splits));
    // the source's image and, behind it, the extra tail
    b->up.ensure(g.o_extra + extra);
    g.enqueue_copies(b->up.p, ctx->up_pin.p, st);
    int64_t* dord = reinterpret_cast<int64_t*>(b->up.as<char>() + g.o_extra);
    FM_HIP_CHECK(hipMemcpyAsync(dord, hord, extra, hipMemcpyHostToDevice, st));
    launch_layout_splits(g.view(b->up.p), dord, dord + n, dord + 2 * n + 1, n_splits, n, b->dev, b->split_rp.as<int64_t>(),
                         st);
    b->host_rp.assign(rp, rp + n + 1);
    b->split_rows.assign(split_rows, split_rows + n_splits + 1);
    FM_HIP_CHECK(hipStreamSynchronize(st));
    b->up.release();  // the source's image: the laid-out dataset alone stays resident
    *out = b.release();
    return FM_OK;
  });
}

int fm_batch_split_view(fm_ctx* ctx, const fm_batch* data, int32_t split, fm_batch** out) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(out != nullptr && data != nullptr, "null argument");
    FM_REQUIRE(data->owner == ctx, "data belongs to another context");
    if (ctx->group) return group_batch_split_view(ctx, data, split, out);
    const int64_t ns = (int64_t)data->split_rows.size() - 1;
    FM_REQUIRE(ns >= 1, "data must be a dataset made by fm_batch_create_splits");
    FM_REQUIRE(split >= 0 && split < ns, "split index out of range");
    OutBatch res = out_batch(ctx, data, out, false);
    fm_batch* b = res.b;
    if (!b->view_of) {
      // an owning batch becomes a view: its own buffers are freed once no queued work reads them
      for (hipEvent_t e : {b->last_use, b->ready, b->built, b->sel_copied})
        if (e) FM_HIP_CHECK(hipEventSynchronize(e));
      for (DevBuf* d : {&b->dev.row_ptr, &b->dev.col, &b->dev.ent, &b->dev.xs, &b->dev.label, &b->up}) d->release();
    }
    b->ensure_events(ctx->stream);
    // the split's rows, entries and labels in place: pointers into data (no copy, no gather); the
    // step's reads of a view are ordered like any batch's (data was complete when it was created)
    const int64_t r0 = data->split_rows[split], r1 = data->split_rows[split + 1];
    const int64_t e0 = data->host_rp[r0], e1 = data->host_rp[r1];
    b->view_of = data;
    b->dev.n_rows = r1 - r0;
    b->dev.nnz = e1 - e0;
    b->dev.row_ptr.borrow(data->split_rp.as<int64_t>() + r0 + split, sizeof(int64_t) * (r1 - r0 + 1));
    b->dev.col.borrow(data->dev.col.as<uint32_t>() + e0, sizeof(uint32_t) * (e1 - e0));
    b->dev.ent.borrow(data->dev.ent.as<uint2>() + e0, sizeof(uint2) * (e1 - e0));
    b->dev.xs.borrow(data->dev.xs.as<float>() + e0, sizeof(float) * (e1 - e0));
    b->dev.label.borrow(data->dev.label.as<double>() + r0, sizeof(double) * (r1 - r0));
    b->max_id = data->max_id;
    b->prepared = false;
    b->host_rp.clear();
    b->row_group = 0;
    res.commit();
    return FM_OK;
  });
}

int32_t fm_fuse_active(fm_ctx* ctx) {
  if (!ctx) return -1;
  // a multi-GPU context never fuses: replicas feed fm_repl_grad the whole sorted view, and a sharded
  // owner's fused step measured slower than the unfused one at R = 8 and at world 1
  if (ctx->group) return 0;
  return fuse_on(ctx) ? 1 : 0;
}

int64_t fm_batch_rows(const fm_batch* b) { return b ? b->dev.n_rows : -1; }
int64_t fm_batch_nnz(const fm_batch* b) { return b ? b->dev.nnz : -1; }
int32_t fm_batch_group(const fm_batch* b) { return b ? b->row_group : -1; }

int fm_batch_set_group(fm_ctx* ctx, fm_batch* b, int32_t group) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(b != nullptr && b->owner == ctx, "batch belongs to another context");
    FM_REQUIRE(!ctx->group && !b->grp, "fm_batch_set_group: a multi-GPU context's batches are cut over its ranks");
    FM_REQUIRE(b->split_rows.empty(), "fm_batch_set_group: a dataset made by fm_batch_create_splits is not grouped");
    FM_REQUIRE(group == 0 || (group >= 2 && group <= 1025), "group must be 0 or in [2, 1025], got " + std::to_string(group));
    FM_REQUIRE(group == 0 || b->dev.n_rows % group == 0,
               "group " + std::to_string(group) + " does not divide the batch's " + std::to_string(b->dev.n_rows) + " rows");
    b->row_group = group;
    return FM_OK;
  });
}

int fm_step_batch(fm_ctx* ctx, fm_batch* batch, int32_t t, double step_size, double reg_param,
                  fm_step_out* out) {
  return guarded(ctx, [&]() -> int {
    if (ctx->group) return group_step_batch(ctx, batch, t, step_size, reg_param, out);
    return step_impl(ctx, batch, t, step_size, reg_param, out);
  });
}

int fm_step(fm_ctx* ctx, const fm_csr* csr, int32_t t, double step_size, double reg_param, fm_step_out* out) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(csr != nullptr, "null batch");
    FM_REQUIRE(ctx->cfg.loss != FM_LOSS_BPR,
               "an FM_LOSS_BPR step needs a grouped batch: a host batch carries no group (fm_batch_sample_pairs, or "
               "fm_batch_create + fm_batch_set_group, then fm_step_batch)");
    if (csr->n_rows == 0) {
      if (out) {
        out->loss_sum = 0.0;
        out->n_rows = 0;
        out->n_loss_rows = 0;
        out->n_unique = 0;
      }
      if (!ctx->group) return FM_NOTHING_TO_DO;  // a group's other processes may hold rows: they agree below
    }
    if (ctx->group) return group_step(ctx, csr, t, step_size, reg_param, out);
    // two upload slots used in turn: while the device runs step i from one slot, the host explodes
    // batch i + 1 into the other slot's pinned staging and its copies queue on the copy stream
    HostSlot& h = ctx->hslot[ctx->hnext];
    ctx->hnext ^= 1;
    if (!h.batch) {
      h.batch.reset(new fm_batch());
      FM_HIP_CHECK(hipEventCreateWithFlags(&h.copied, hipEventDisableTiming));
      FM_HIP_CHECK(hipEventCreateWithFlags(&h.consumed, hipEventDisableTiming));
      FM_HIP_CHECK(hipEventRecord(h.copied, ctx->stream));
      FM_HIP_CHECK(hipEventRecord(h.consumed, ctx->stream));
    }
    if (!ctx->copy_stream) FM_HIP_CHECK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    FM_HIP_CHECK(hipEventSynchronize(h.copied));  // the slot's staging has been copied out
    const Staged g = stage_csr(ctx, csr, true, h.pin);
    if (!batch_fits(h.batch.get(), g)) FM_HIP_CHECK(hipEventSynchronize(h.consumed));  // before reallocating
    FM_HIP_CHECK(hipStreamWaitEvent(ctx->copy_stream, h.consumed, 0));  // the slot's last step read it
    copy_staged(ctx, g, h.pin, h.batch.get(), ctx->copy_stream);
    FM_HIP_CHECK(hipEventRecord(h.copied, ctx->copy_stream));
    FM_HIP_CHECK(hipStreamWaitEvent(ctx->stream, h.copied, 0));
    const int rc = step_impl(ctx, h.batch.get(), t, step_size, reg_param, out);  // out == NULL: no host sync
    FM_HIP_CHECK(hipEventRecord(h.consumed, ctx->stream));
    return rc;
  });
}

int fm_loss_history(fm_ctx* ctx, double* loss, int64_t cap, int64_t* n) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(n != nullptr, "null n");
    if (ctx->group) return group_loss_history(ctx, loss, cap, n);
    *n = ctx->epoch;
    if (cap == 0 || ctx->epoch == 0) return FM_OK;
    FM_REQUIRE(loss != nullptr, "null loss buffer");
    const int64_t m = std::min<int64_t>(cap, ctx->epoch);
    std::vector<double> h(3 * m);
    FM_HIP_CHECK(hipMemcpyAsync(h.data(), ctx->loss_hist.p, sizeof(double) * 3 * m, hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < m; ++i) loss[i] = h[3 * i];
    return FM_OK;
  });
}

int fm_predict(fm_ctx* ctx, const fm_csr* csr, double lo, double hi, double* pred) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(csr != nullptr && (csr->n_rows == 0 || pred), "null argument");
    if (ctx->group) return group_predict(ctx, csr, lo, hi, pred);
    if (csr->n_rows == 0) return FM_OK;
    fm_batch* b = host_batch(ctx);
    upload_batch(ctx, csr, b, false);
    DevBuf dp;
    dp.ensure(sizeof(double) * csr->n_rows);
    launch_predict(ctx->view(), b->dev, ctx->cum_host.back(), ctx->cfg.w0, lo, hi, dp.as<double>(), ctx->stream);
    FM_HIP_CHECK(hipMemcpyAsync(pred, dp.p, sizeof(double) * csr->n_rows, hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return FM_OK;
  });
}

int fm_predict_batch(fm_ctx* ctx, fm_batch* b, double lo, double hi, double* pred) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(b != nullptr && b->owner == ctx, "batch belongs to another context");
    if (ctx->group) return group_predict_batch(ctx, b, lo, hi, pred);
    const int64_t B = b->dev.n_rows;
    FM_REQUIRE(B == 0 || pred, "null argument");
    if (B == 0) return FM_OK;
    DevBuf dp;
    dp.ensure(sizeof(double) * B);
    wait_built(b, ctx->stream);
    hipEvent_t e0 = ctx->prof_begin(ctx->stream);
    launch_predict(ctx->view(), b->dev, ctx->cum_host.back(), ctx->cfg.w0, lo, hi, dp.as<double>(), ctx->stream);
    ctx->prof_end("predict", e0, ctx->stream);
    FM_HIP_CHECK(hipMemcpyAsync(pred, dp.p, sizeof(double) * B, hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    return FM_OK;
  });
}

// One evaluation of a single-table context's batch on the main stream: the forward in kEvaluate mode,
// the fold into the history's next slot, the record counted; pred / out as fm_evaluate_batch takes them.
static int evaluate_impl(fm_ctx* ctx, fm_batch* b, double lo, double hi, double* pred, fm_eval_out* out) {
  const int64_t B = b->dev.n_rows;
  hipStream_t st = ctx->stream;
  double* slot = eval_next_slot(ctx);
  if (pred) ctx->eval_pred.ensure_slack(sizeof(double) * B);
  wait_built(b, st);
  hipEvent_t e0 = ctx->prof_begin(st);
  const int64_t nblk = launch_evaluate(ctx->view(), b->dev, ctx->work, ctx->cum_host.back(), ctx->cfg.w0, lo, hi,
                                       pred ? ctx->eval_pred.as<double>() : nullptr, st);
  hipEvent_t ef = ctx->prof_begin(st);  // the fold alone, inside "evaluate"
  launch_eval_fold(ctx->work.eval_part.as<double>(), nblk, slot, st);
  ctx->prof_end("eval_fold", ef, st);
  ctx->prof_end("evaluate", e0, st);
  // a read of the batch: its next fm_batch_prepare or fm_batch_from_rows refill waits for it
  if (b->last_use) FM_HIP_CHECK(hipEventRecord(b->last_use, st));
  if (pred) FM_HIP_CHECK(hipMemcpyAsync(pred, ctx->eval_pred.p, sizeof(double) * B, hipMemcpyDeviceToHost, st));
  eval_commit(ctx, out);
  return FM_OK;
}

int fm_evaluate(fm_ctx* ctx, const fm_csr* csr, double lo, double hi, double* pred, fm_eval_out* out) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(csr != nullptr && out != nullptr, "null argument");
    *out = fm_eval_out{};
    if (ctx->group) return group_evaluate(ctx, csr, lo, hi, pred, out);
    if (csr->n_rows == 0) return FM_NOTHING_TO_DO;
    fm_batch* b = host_batch(ctx);
    upload_batch(ctx, csr, b, false);
    return evaluate_impl(ctx, b, lo, hi, pred, out);
  });
}

int fm_evaluate_batch(fm_ctx* ctx, fm_batch* b, double lo, double hi, double* pred, fm_eval_out* out) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(b != nullptr && b->owner == ctx, "batch belongs to another context");
    FM_REQUIRE(out != nullptr || pred == nullptr, "pred needs out: an evaluation that only enqueues returns no predictions");
    FM_REQUIRE(b->split_rows.empty(), "a dataset made by fm_batch_create_splits is evaluated by split");
    if (out) *out = fm_eval_out{};
    if (ctx->group) return group_evaluate_batch(ctx, b, lo, hi, pred, out);
    if (b->dev.n_rows == 0) return FM_NOTHING_TO_DO;
    return evaluate_impl(ctx, b, lo, hi, pred, out);
  });
}

int fm_eval_history(fm_ctx* ctx, fm_eval_out* out, int64_t cap, int64_t* n) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(n != nullptr, "null n");
    if (ctx->group) {  // the ranks' summed records, kept on the host
      *n = (int64_t)ctx->eval_host.size();
      if (cap == 0 || *n == 0) return FM_OK;
      FM_REQUIRE(out != nullptr, "null history buffer");
      std::copy_n(ctx->eval_host.begin(), std::min<int64_t>(cap, *n), out);
      return FM_OK;
    }
    *n = ctx->eval_n;
    if (cap == 0 || ctx->eval_n == 0) return FM_OK;
    FM_REQUIRE(out != nullptr, "null history buffer");
    const int64_t m = std::min<int64_t>(cap, ctx->eval_n);
    std::vector<double> h(kEvalRec * m);
    FM_HIP_CHECK(hipMemcpyAsync(h.data(), ctx->eval_hist.p, sizeof(double) * kEvalRec * m, hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < m; ++i) eval_read(h.data() + kEvalRec * i, ctx->eval_epoch[i], out + i);
    return FM_OK;
  });
}

// ---- binary evaluation (fm_binary_metrics, fm_evaluate_binary[_batch], fm_eval_binary_history; fm_binary.hip) ----
static void binary_read(const int64_t* rec, int64_t epoch, fm_binary_out* out) {
  out->n_rows = rec[0];
  out->n_pos = rec[1];
  out->epoch = epoch;
  out->tp = rec[2];
  out->fp = rec[3];
  out->two_u = rec[4];
  std::memcpy(&out->sum_log_loss, &rec[5], sizeof(double));
}

// a single-table context that holds the whole table: the binary evaluation is single-GPU, as the logistic step
static void require_binary_ctx(const fm_ctx* ctx, const char* call) {
  FM_REQUIRE(!ctx->group && ctx->cfg.shard_count == 1,
             std::string(call) + " needs a single-table context: multi-GPU and sharded (shard_count > 1) contexts have no "
                                 "binary evaluation");
}

// the stage over n device scores and labels into rec (device), on the main stream (profile "evaluate_binary",
// its sort and its count -- scan, pair count, fold -- inside it); e0: a profile start recorded by the caller
// ahead of its score pass, or null
static void binary_stage(fm_ctx* ctx, const double* score, const double* label, int64_t n, int64_t* rec, hipEvent_t e0) {
  hipStream_t st = ctx->stream;
  BinaryWork& w = ctx->binary;
  w.ensure(n);
  if (!e0) e0 = ctx->prof_begin(st);
  launch_binary_rows(w, score, label, n, st);
  hipEvent_t es = ctx->prof_begin(st);
  launch_binary_sort(w, n, st);
  ctx->prof_end("binary_sort", es, st);
  hipEvent_t ec = ctx->prof_begin(st);
  launch_binary_count(w, n, rec, st);
  ctx->prof_end("binary_count", ec, st);
  ctx->prof_end("evaluate_binary", e0, st);
}

// the record at rec (device) read back: the main stream is waited for
static void binary_fetch(fm_ctx* ctx, const int64_t* rec, fm_binary_out* out) {
  ctx->pinned.ensure(64);
  FM_HIP_CHECK(hipMemcpyAsync(ctx->pinned.p, rec, sizeof(int64_t) * kBinaryRec, hipMemcpyDeviceToHost, ctx->stream));
  FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  binary_read(reinterpret_cast<const int64_t*>(ctx->pinned.p), ctx->epoch, out);
}

int fm_binary_metrics(fm_ctx* ctx, const double* score, const double* label, int64_t n, fm_binary_out* out) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(out != nullptr, "fm_binary_metrics: null out");
    *out = fm_binary_out{};
    require_binary_ctx(ctx, "fm_binary_metrics");
    FM_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "fm_binary_metrics: n out of range");
    if (n == 0) return FM_NOTHING_TO_DO;
    FM_REQUIRE(score != nullptr && label != nullptr, "fm_binary_metrics: null score or label");
    BinaryWork& w = ctx->binary;
    w.score.ensure_slack(sizeof(double) * (size_t)n);
    w.label.ensure_slack(sizeof(double) * (size_t)n);
    w.rec.ensure(sizeof(int64_t) * kBinaryRec);
    // (pageable host memory: the copies have left the caller's buffers when they return)
    FM_HIP_CHECK(hipMemcpyAsync(w.score.p, score, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    FM_HIP_CHECK(hipMemcpyAsync(w.label.p, label, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
    binary_stage(ctx, w.score.as<double>(), w.label.as<double>(), n, w.rec.as<int64_t>(), nullptr);
    binary_fetch(ctx, w.rec.as<int64_t>(), out);
    return FM_OK;
  });
}

// One binary evaluation of a single-table context's batch on the main stream: launch_predict's unclamped
// score of every row, the stage against the batch's labels into the history's next slot, the record counted;
// score / out as fm_evaluate_binary_batch takes them.
static int evaluate_binary_impl(fm_ctx* ctx, fm_batch* b, double* score, fm_binary_out* out) {
  const int64_t B = b->dev.n_rows;
  FM_REQUIRE(B < (int64_t(1) << 31), "fm_evaluate_binary: too many rows");
  hipStream_t st = ctx->stream;
  BinaryWork& w = ctx->binary;
  ctx->ensure_bin_hist(ctx->bin_n + 1);
  int64_t* slot = ctx->bin_hist.as<int64_t>() + kBinaryRec * ctx->bin_n;
  w.score.ensure_slack(sizeof(double) * (size_t)B);
  w.ensure(B);
  wait_built(b, st);
  hipEvent_t e0 = ctx->prof_begin(st);
  const double inf = std::numeric_limits<double>::infinity();
  launch_predict(ctx->view(), b->dev, ctx->cum_host.back(), ctx->cfg.w0, -inf, inf, w.score.as<double>(), st);
  binary_stage(ctx, w.score.as<double>(), b->dev.label.as<double>(), B, slot, e0);
  // a read of the batch: its next fm_batch_prepare or fm_batch_from_rows refill waits for it
  if (b->last_use) FM_HIP_CHECK(hipEventRecord(b->last_use, st));
  if (score) FM_HIP_CHECK(hipMemcpyAsync(score, w.score.p, sizeof(double) * (size_t)B, hipMemcpyDeviceToHost, st));
  ctx->bin_epoch.push_back(ctx->epoch);
  ctx->bin_n += 1;
  if (out) binary_fetch(ctx, slot, out);
  return FM_OK;
}

int fm_evaluate_binary(fm_ctx* ctx, const fm_csr* csr, double* score, fm_binary_out* out) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(csr != nullptr && out != nullptr, "fm_evaluate_binary: null argument");
    *out = fm_binary_out{};
    require_binary_ctx(ctx, "fm_evaluate_binary");
    if (csr->n_rows == 0) return FM_NOTHING_TO_DO;
    fm_batch* b = host_batch(ctx);
    upload_batch(ctx, csr, b, false);
    return evaluate_binary_impl(ctx, b, score, out);
  });
}

int fm_evaluate_binary_batch(fm_ctx* ctx, fm_batch* b, double* score, fm_binary_out* out) {
  return guarded(ctx, [&]() -> int {
    if (out) *out = fm_binary_out{};
    FM_REQUIRE(b != nullptr && b->owner == ctx, "fm_evaluate_binary_batch: batch belongs to another context");
    FM_REQUIRE(out != nullptr || score == nullptr,
               "fm_evaluate_binary_batch: score needs out: an evaluation that only enqueues returns no scores");
    FM_REQUIRE(b->split_rows.empty(),
               "fm_evaluate_binary_batch: a dataset made by fm_batch_create_splits is evaluated by split");
    require_binary_ctx(ctx, "fm_evaluate_binary_batch");
    if (b->dev.n_rows == 0) return FM_NOTHING_TO_DO;
    return evaluate_binary_impl(ctx, b, score, out);
  });
}

int fm_eval_binary_history(fm_ctx* ctx, fm_binary_out* out, int64_t cap, int64_t* n) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(n != nullptr, "fm_eval_binary_history: null n");
    *n = ctx->bin_n;
    if (cap <= 0 || ctx->bin_n == 0) return FM_OK;
    FM_REQUIRE(out != nullptr, "fm_eval_binary_history: null history buffer");
    const int64_t m = std::min<int64_t>(cap, ctx->bin_n);
    std::vector<int64_t> h(kBinaryRec * m);
    FM_HIP_CHECK(hipMemcpyAsync(h.data(), ctx->bin_hist.p, sizeof(int64_t) * kBinaryRec * m, hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < m; ++i) binary_read(h.data() + kBinaryRec * i, ctx->bin_epoch[i], out + i);
    return FM_OK;
  });
}

// ---- ranking (fm_rank_candidates / fm_rank_batch, their _select forms, fm_rank_positions[_batch]; fm_rank.hip) ----
// a replicated group's replicas are identical: member 0 answers, with the group locked (as fm_loss_grad).
// repeat(member 0): the same call on it.  (A template inside this file's extern "C" block takes C++ linkage by name.)
extern "C++" template <class F>
static int rank_on_member0(fm_ctx* ctx, F&& repeat) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(ctx->cfg.parallel == FM_PARALLEL_REPLICATED,
               "fm_rank needs the whole table on one device (a replicated or single-table context): a row-sharded "
               "table is not ranked yet");
    return repeat(group_member0(ctx));
  });
}

// The two row sets of a call, as host rows or as batches of the context.  rank_rows_check: what is refused
// whatever else the call asks (call / host_call: the batch form's name and its host-row form's, for the
// message), and the sets' sizes.  rank_rows_ready, behind the call's own checks: both sets on the device.
struct RankRows {
  const BatchDev& u;
  const BatchDev& c;
};
static std::pair<int64_t, int64_t> rank_rows_check(const fm_ctx*, const fm_csr* contexts, const fm_csr* candidates, const char*,
                                                   const char*) {
  FM_REQUIRE(contexts != nullptr && candidates != nullptr, "null argument");
  return {contexts->n_rows, candidates->n_rows};
}
static std::pair<int64_t, int64_t> rank_rows_check(const fm_ctx* ctx, const fm_batch* contexts, const fm_batch* candidates,
                                                   const char* call, const char* host_call) {
  FM_REQUIRE(contexts != nullptr && candidates != nullptr, "null argument");
  FM_REQUIRE(contexts->owner == ctx && candidates->owner == ctx, "batch belongs to another context");
  FM_REQUIRE(!ctx->group && !contexts->grp && !candidates->grp,
             std::string(call) + " needs both row sets whole on one device: a multi-GPU context's batches are cut over its "
                                 "ranks (" + host_call + " takes host rows)");
  FM_REQUIRE(contexts->split_rows.empty() && candidates->split_rows.empty(),
             "a dataset made by fm_batch_create_splits is ranked through its split views");
  return {contexts->dev.n_rows, candidates->dev.n_rows};
}
static RankRows rank_rows_ready(fm_ctx* ctx, const fm_csr* contexts, const fm_csr* candidates) {
  fm_batch* bu = host_batch(ctx);
  if (!ctx->host_batch2) ctx->host_batch2.reset(new fm_batch());
  fm_batch* bc = ctx->host_batch2.get();
  upload_batch(ctx, contexts, bu, false);
  upload_batch(ctx, candidates, bc, false);
  return {bu->dev, bc->dev};
}
static RankRows rank_rows_ready(fm_ctx* ctx, const fm_batch* contexts, const fm_batch* candidates) {
  wait_built(contexts, ctx->stream);
  wait_built(candidates, ctx->stream);
  return {contexts->dev, candidates->dev};
}

// the argument rules every ranking call shares, for U contexts and Cn candidates; false: nothing to do
static bool rank_common_check(const fm_ctx* ctx, int64_t U, int64_t Cn) {
  FM_REQUIRE(ctx->cfg.shard_count == 1,
             "fm_rank needs the whole table on one device (shard_count == 1): a row-sharded table is not ranked yet");
  if (U == 0) return false;
  FM_REQUIRE(Cn >= 1, "fm_rank needs at least one candidate row");
  FM_REQUIRE(Cn < (int64_t(1) << 31), "fm_rank takes fewer than 2^31 candidate rows");
  return true;
}

// The rules of one set of per-context row lists (ptr[U + 1], rows[ptr[U]]; ptr not null) for Cn candidates,
// in one pass over the host arrays, before anything is enqueued or sized: returns the longest list.
// what: put before every message (the list's name where a call takes several); pname / rname: the
// arguments' names.
static int64_t rank_list_check(const std::string& what, const std::string& pname, const std::string& rname,
                               const int64_t* ptr, const int32_t* rows, int64_t U, int64_t Cn) {
  FM_REQUIRE(ptr[0] == 0, what + pname + "[0] must be 0, got " + std::to_string(ptr[0]));
  for (int64_t u = 0; u < U; ++u) {
    FM_REQUIRE(ptr[u + 1] >= ptr[u], what + pname + " must be non-decreasing: " + pname + "[" + std::to_string(u + 1) +
                                         "] < " + pname + "[" + std::to_string(u) + "]");
    FM_REQUIRE(ptr[u + 1] < (int64_t(1) << 31), what + pname + "[" + std::to_string(u + 1) + "] must be < 2^31");
  }
  FM_REQUIRE(ptr[U] == 0 || rows != nullptr, what + "null " + rname + " with a list that is not empty");
  // The rows, context chunk after context chunk on the pool's threads once the lists are long (fm_batch_sample_pairs
  // hands over every context's list at every call: 13.1M rows took 9.7 ms on one thread, tools/pair_bench.py); a
  // few short lists run inline.  Each chunk stops at its first offending entry; the lowest one is reported, as by
  // one pass in order.
  const int64_t T = std::min<int64_t>(chunk_count(ptr[U], int64_t(1) << 18), std::max<int64_t>(U, 1));
  std::vector<int64_t> bad_u(T, -1), bad_e(T, -1), longest_of(T, 0);
  parallel_chunks_t(U, T, [&](int64_t t, int64_t u0, int64_t u1) {
    int64_t lg = 0;
    for (int64_t u = u0; u < u1; ++u) {
      for (int64_t e = ptr[u]; e < ptr[u + 1]; ++e) {
        const int64_t r = rows[e];
        const bool in_range = r >= 0 && r < Cn, in_order = e == ptr[u] || rows[e - 1] < r;
        if (in_range && in_order) continue;
        bad_u[t] = u;
        bad_e[t] = e;
        return;
      }
      lg = std::max(lg, ptr[u + 1] - ptr[u]);
    }
    longest_of[t] = lg;
  });
  int64_t longest = 0;
  for (int64_t t = 0; t < T; ++t) {
    if (bad_u[t] >= 0) {
      const int64_t u = bad_u[t], e = bad_e[t], r = rows[e];
      const bool in_range = r >= 0 && r < Cn;
      const std::string at = what + "context " + std::to_string(u) + ", position " + std::to_string(e - ptr[u]) + ": row " +
                             std::to_string(r);
      FM_REQUIRE(in_range, at + " is out of range [0, " + std::to_string(Cn) + ")");
      FM_REQUIRE(false, at + " after row " + std::to_string(rows[e - 1]) + ": a list must be strictly ascending");
    }
    longest = std::max(longest, longest_of[t]);
  }
  return longest;
}

// a checked list pair -> its device copy (offsets [U + 1], rows)
static void upload_lists(DevBuf& ptr, DevBuf& rows, const int64_t* host_ptr, const int32_t* host_rows, int64_t U,
                         hipStream_t st) {
  const size_t n = (size_t)host_ptr[U];
  ptr.ensure_slack(sizeof(int64_t) * (size_t)(U + 1));
  rows.ensure_slack(sizeof(int32_t) * n);
  FM_HIP_CHECK(hipMemcpyAsync(ptr.p, host_ptr, sizeof(int64_t) * (size_t)(U + 1), hipMemcpyHostToDevice, st));
  if (n) FM_HIP_CHECK(hipMemcpyAsync(rows.p, host_rows, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
}

// where a call's lists are on the device: an fm_lists' own buffers as they stand, or the host arrays' copy
// in the context's scratch (ptr / rows), enqueued here; {null, null} without lists
struct DevLists {
  const int64_t* ptr = nullptr;
  const int32_t* rows = nullptr;
};
static DevLists device_lists(DevBuf& ptr, DevBuf& rows, const RankList& l, int64_t U, hipStream_t st) {
  if (l.dev_ptr) return {l.dev_ptr, l.dev_rows};
  if (!l.ptr) return {};
  upload_lists(ptr, rows, l.ptr, l.rows, U, st);
  return {ptr.as<int64_t>(), rows.as<int32_t>()};
}

// An fm_lists as a call's lists, for U contexts and Cn candidates: of this context and of these sizes (what:
// the argument's name).  Its rules were checked when it was made; nothing of it is read here but its sizes.
static RankList resident_list(const fm_ctx* ctx, const fm_lists* l, int64_t U, int64_t Cn, const char* what) {
  FM_REQUIRE(l->owner == ctx, std::string(what) + ": the lists belong to another context");
  FM_REQUIRE(l->U == U, std::string(what) + ": lists of " + std::to_string(l->U) + " contexts for contexts of " +
                            std::to_string(U) + " rows");
  FM_REQUIRE(l->C == Cn, std::string(what) + ": lists over " + std::to_string(l->C) + " candidate rows for candidates of " +
                             std::to_string(Cn) + " rows");
  return {l->host_ptr.data(), nullptr, l->longest, l->ptr.as<int64_t>(), l->rows.as<int32_t>()};
}

// The stage every ranking call opens with: both row sets' summaries and biases into the context's scratch
// (one profile entry), as the views the score and position launchers take.
static std::pair<RankSide, RankSide> rank_summaries(fm_ctx* ctx, const BatchDev& bu, const BatchDev& bc) {
  const int64_t U = bu.n_rows, Cn = bc.n_rows;
  const int kp = ctx->kp;
  RankWork& w = ctx->rank;
  const size_t srow = sizeof(double) * (size_t)(kp + 2);
  w.sum_u.ensure_slack(srow * U);
  w.sum_c.ensure_slack(srow * Cn);
  w.cnt_u.ensure_slack(sizeof(uint32_t) * U);
  w.cnt_c.ensure_slack(sizeof(uint32_t) * Cn);
  w.bias_u.ensure_slack(sizeof(double) * U);
  w.bias_c.ensure_slack(sizeof(double) * Cn);
  const TableView T = ctx->view();
  const double cumE = ctx->cum_host.back();
  hipStream_t st = ctx->stream;
  hipEvent_t e0 = ctx->prof_begin(st);
  launch_summary(T, bu, cumE, w.sum_u.as<double>(), w.cnt_u.as<uint32_t>(), st);
  launch_summary(T, bc, cumE, w.sum_c.as<double>(), w.cnt_c.as<uint32_t>(), st);
  launch_rank_bias(w.sum_u.as<double>(), U, kp, w.bias_u.as<double>(), st);
  launch_rank_bias(w.sum_c.as<double>(), Cn, kp, w.bias_c.as<double>(), st);
  ctx->prof_end("rank_summary", e0, st);
  return {RankSide{w.sum_u.as<double>(), w.bias_u.as<double>(), w.cnt_u.as<uint32_t>(), U},
          RankSide{w.sum_c.as<double>(), w.bias_c.as<double>(), w.cnt_c.as<uint32_t>(), Cn}};
}

// Top-N on one whole table: the lists' copy and the summaries, then the score and merge passes over the
// contexts in tiles whose split lists fit the budget (fm_rank.hip).  select / sel: the mode and lists of the
// _select calls (checked by rank_call); FM_RANK_SELECT_ALL reads no list.
static int rank_impl(fm_ctx* ctx, const RankRows& rows, int32_t n_top, double lo, double hi, int32_t* top_index,
                     double* top_score, int32_t select, const RankList& sel) {
  const int64_t U = rows.u.n_rows, Cn = rows.c.n_rows;
  const int kp = ctx->kp;
  const double w0 = ctx->cfg.w0;
  RankWork& w = ctx->rank;
  hipStream_t st = ctx->stream;
  // FM_RANK_SELECT_ONLY cuts each context's list, not the candidates: the longest list sets the splits
  const int splits = rank_splits(select == FM_RANK_SELECT_ONLY ? sel.longest : Cn, U);
  const int64_t tile = std::min<int64_t>(U, rank_ctx_tile(splits, n_top));
  w.lkey.ensure_slack(sizeof(uint64_t) * (size_t)(tile * splits * n_top));
  w.lidx.ensure_slack(sizeof(uint32_t) * (size_t)(tile * splits * n_top));
  w.out_idx.ensure_slack(sizeof(int32_t) * (size_t)(U * n_top));
  w.out_score.ensure_slack(sizeof(double) * (size_t)(U * n_top));
  const DevLists dsel = device_lists(w.sel_ptr, w.sel_rows, sel, U, st);
  const auto [su, sc] = rank_summaries(ctx, rows.u, rows.c);
  for (int64_t u0 = 0; u0 < U; u0 += tile) {
    const int64_t Ut = std::min<int64_t>(tile, U - u0);
    hipEvent_t e0 = ctx->prof_begin(st);
    // the tile's offsets: sel_ptr + u0 (they index the whole call's sel_rows)
    launch_rank_score(select, su.tile(u0, Ut, kp), sc, dsel.ptr ? dsel.ptr + u0 : nullptr, dsel.rows, kp, splits, n_top, w0,
                      w.lkey.as<uint64_t>(), w.lidx.as<uint32_t>(), st);
    ctx->prof_end("rank_score", e0, st);
    e0 = ctx->prof_begin(st);
    launch_rank_merge(w.lkey.as<uint64_t>(), w.lidx.as<uint32_t>(), Ut, splits, n_top, su.cnt + u0, sc.cnt, w0, lo, hi,
                      w.out_idx.as<int32_t>() + u0 * n_top, w.out_score.as<double>() + u0 * n_top, st);
    ctx->prof_end("rank_merge", e0, st);
  }
  FM_HIP_CHECK(hipMemcpyAsync(top_index, w.out_idx.p, sizeof(int32_t) * (size_t)(U * n_top), hipMemcpyDeviceToHost, st));
  FM_HIP_CHECK(hipMemcpyAsync(top_score, w.out_score.p, sizeof(double) * (size_t)(U * n_top), hipMemcpyDeviceToHost, st));
  FM_HIP_CHECK(hipStreamSynchronize(st));
  return FM_OK;
}

// The top-N entry points over either kind of row set: the shared rules, the top-N rules, the list
// rules of the _select forms (rank_list_check; FM_RANK_SELECT_ALL takes no list) or -- resident -- the
// fm_lists' fit (resident_list: checked when it was made), then the work.
extern "C++" template <class Rows>
static int rank_call(fm_ctx* ctx, const Rows* contexts, const Rows* candidates, const char* call, const char* host_call,
                     int32_t select, const int64_t* sel_ptr, const int32_t* sel_rows, int32_t n_top, double lo, double hi,
                     int32_t* top_index, double* top_score, bool resident = false, const fm_lists* rsel = nullptr) {
  return guarded(ctx, [&]() -> int {
    const auto [U, Cn] = rank_rows_check(ctx, contexts, candidates, call, host_call);
    if (!rank_common_check(ctx, U, Cn)) return FM_OK;
    FM_REQUIRE(n_top >= 1 && n_top <= FM_RANK_MAX_TOP && n_top <= Cn, "n_top must be in [1, min(candidate rows, FM_RANK_MAX_TOP)]");
    FM_REQUIRE(top_index != nullptr && top_score != nullptr, "null argument");
    FM_REQUIRE(select == FM_RANK_SELECT_ALL || select == FM_RANK_SELECT_ONLY || select == FM_RANK_SELECT_EXCEPT,
               "select must be FM_RANK_SELECT_ALL, _ONLY or _EXCEPT, got " + std::to_string(select));
    RankList sel;
    if (select != FM_RANK_SELECT_ALL && resident) {
      FM_REQUIRE(rsel != nullptr, "null sel with FM_RANK_SELECT_ONLY / _EXCEPT");
      sel = resident_list(ctx, rsel, U, Cn, "sel");
    } else if (select != FM_RANK_SELECT_ALL) {
      FM_REQUIRE(sel_ptr != nullptr, "null sel_ptr with FM_RANK_SELECT_ONLY / _EXCEPT");
      sel = {sel_ptr, sel_rows, rank_list_check("", "sel_ptr", "sel_rows", sel_ptr, sel_rows, U, Cn)};
    }
    return rank_impl(ctx, rank_rows_ready(ctx, contexts, candidates), n_top, lo, hi, top_index, top_score, select, sel);
  });
}

int fm_rank_candidates_select(fm_ctx* ctx, const fm_csr* contexts, const fm_csr* candidates, int32_t select,
                              const int64_t* sel_ptr, const int32_t* sel_rows, int32_t n_top, double lo, double hi,
                              int32_t* top_index, double* top_score) {
  if (ctx && ctx->group)
    return rank_on_member0(ctx, [&](fm_ctx* m) {
      return fm_rank_candidates_select(m, contexts, candidates, select, sel_ptr, sel_rows, n_top, lo, hi, top_index, top_score);
    });
  return rank_call(ctx, contexts, candidates, "", "", select, sel_ptr, sel_rows, n_top, lo, hi, top_index, top_score);
}

int fm_rank_batch_select(fm_ctx* ctx, fm_batch* contexts, fm_batch* candidates, int32_t select, const int64_t* sel_ptr,
                         const int32_t* sel_rows, int32_t n_top, double lo, double hi, int32_t* top_index,
                         double* top_score) {
  return rank_call<fm_batch>(ctx, contexts, candidates, "fm_rank_batch", "fm_rank_candidates", select, sel_ptr, sel_rows, n_top,
                             lo, hi, top_index, top_score);
}

int fm_rank_batch_select_lists(fm_ctx* ctx, fm_batch* contexts, fm_batch* candidates, int32_t select, const fm_lists* sel,
                               int32_t n_top, double lo, double hi, int32_t* top_index, double* top_score) {
  return rank_call<fm_batch>(ctx, contexts, candidates, "fm_rank_batch", "fm_rank_candidates", select, nullptr, nullptr, n_top,
                             lo, hi, top_index, top_score, true, sel);
}

int fm_rank_candidates(fm_ctx* ctx, const fm_csr* contexts, const fm_csr* candidates, int32_t n_top, double lo, double hi,
                       int32_t* top_index, double* top_score) {
  return fm_rank_candidates_select(ctx, contexts, candidates, FM_RANK_SELECT_ALL, nullptr, nullptr, n_top, lo, hi, top_index,
                                   top_score);
}

int fm_rank_batch(fm_ctx* ctx, fm_batch* contexts, fm_batch* candidates, int32_t n_top, double lo, double hi,
                  int32_t* top_index, double* top_score) {
  return fm_rank_batch_select(ctx, contexts, candidates, FM_RANK_SELECT_ALL, nullptr, nullptr, n_top, lo, hi, top_index,
                              top_score);
}

// Exact positions on one whole table: the lists' copies and the summaries as rank_impl's, then the counting
// pass over the contexts, a launch per rank_position_ctx_tile() of them (fm_rank.hip).  No scratch but the
// lists' copies and the results: the splits add their counts onto the zeroed positions.  ex.ptr null:
// nothing excluded.
static int rank_positions_impl(fm_ctx* ctx, const RankRows& rows, const RankList& tgt, const RankList& ex, double lo, double hi,
                               int32_t* position, double* score) {
  const int64_t U = rows.u.n_rows, Cn = rows.c.n_rows;
  const int kp = ctx->kp;
  const size_t n_tgt = (size_t)tgt.ptr[U];
  RankWork& w = ctx->rank;
  hipStream_t st = ctx->stream;
  w.position.ensure_slack(sizeof(int32_t) * n_tgt);
  w.pos_score.ensure_slack(sizeof(double) * n_tgt);
  const DevLists dtgt = device_lists(w.tgt_ptr, w.tgt_rows, tgt, U, st);
  const DevLists dex = device_lists(w.sel_ptr, w.sel_rows, ex, U, st);
  FM_HIP_CHECK(hipMemsetAsync(w.position.p, 0, sizeof(int32_t) * n_tgt, st));
  const auto [su, sc] = rank_summaries(ctx, rows.u, rows.c);
  const int splits = rank_splits(Cn, U);
  const int64_t tile = rank_position_ctx_tile();
  for (int64_t u0 = 0; u0 < U; u0 += tile) {
    const int64_t Ut = std::min<int64_t>(tile, U - u0);
    hipEvent_t e0 = ctx->prof_begin(st);
    // the tile's offsets: tgt_ptr + u0, sel_ptr + u0 (they index the whole call's rows and results)
    launch_rank_position(su.tile(u0, Ut, kp), sc, dtgt.ptr + u0, dtgt.rows, tgt.longest, dex.ptr ? dex.ptr + u0 : nullptr,
                         dex.rows, kp, splits, ctx->cfg.w0, lo, hi, w.position.as<int32_t>(), w.pos_score.as<double>(), st);
    ctx->prof_end("rank_position", e0, st);
  }
  FM_HIP_CHECK(hipMemcpyAsync(position, w.position.p, sizeof(int32_t) * n_tgt, hipMemcpyDeviceToHost, st));
  FM_HIP_CHECK(hipMemcpyAsync(score, w.pos_score.p, sizeof(double) * n_tgt, hipMemcpyDeviceToHost, st));
  FM_HIP_CHECK(hipStreamSynchronize(st));
  return FM_OK;
}

// the two positions entry points over either kind of row set, as rank_call
extern "C++" template <class Rows>
static int rank_positions_call(fm_ctx* ctx, const Rows* contexts, const Rows* candidates, const char* call,
                               const char* host_call, const int64_t* tgt_ptr, const int32_t* tgt_rows, const int64_t* excl_ptr,
                               const int32_t* excl_rows, double lo, double hi, int32_t* position, double* score,
                               bool resident = false, const fm_lists* rtgt = nullptr, const fm_lists* rex = nullptr) {
  return guarded(ctx, [&]() -> int {
    const auto [U, Cn] = rank_rows_check(ctx, contexts, candidates, call, host_call);
    if (!rank_common_check(ctx, U, Cn)) return FM_OK;
    FM_REQUIRE(position != nullptr && score != nullptr, "null argument");
    RankList tgt, ex;
    if (resident) {
      FM_REQUIRE(rtgt != nullptr, "null tgt: fm_rank_positions needs the target lists");
      tgt = resident_list(ctx, rtgt, U, Cn, "tgt");
      if (rex) ex = resident_list(ctx, rex, U, Cn, "excl");
    } else {
      FM_REQUIRE(tgt_ptr != nullptr, "null tgt_ptr: fm_rank_positions needs the target lists");
      tgt = {tgt_ptr, tgt_rows, rank_list_check("target list: ", "tgt_ptr", "tgt_rows", tgt_ptr, tgt_rows, U, Cn)};
      if (excl_ptr) ex = {excl_ptr, excl_rows, rank_list_check("exclude list: ", "excl_ptr", "excl_rows", excl_ptr, excl_rows, U, Cn)};
    }
    if (tgt.ptr[U] == 0) return FM_OK;
    return rank_positions_impl(ctx, rank_rows_ready(ctx, contexts, candidates), tgt, ex, lo, hi, position, score);
  });
}

int fm_rank_positions(fm_ctx* ctx, const fm_csr* contexts, const fm_csr* candidates, const int64_t* tgt_ptr,
                      const int32_t* tgt_rows, const int64_t* excl_ptr, const int32_t* excl_rows, double lo, double hi,
                      int32_t* position, double* score) {
  if (ctx && ctx->group)
    return rank_on_member0(ctx, [&](fm_ctx* m) {
      return fm_rank_positions(m, contexts, candidates, tgt_ptr, tgt_rows, excl_ptr, excl_rows, lo, hi, position, score);
    });
  return rank_positions_call(ctx, contexts, candidates, "", "", tgt_ptr, tgt_rows, excl_ptr, excl_rows, lo, hi, position, score);
}

int fm_rank_positions_batch(fm_ctx* ctx, fm_batch* contexts, fm_batch* candidates, const int64_t* tgt_ptr,
                            const int32_t* tgt_rows, const int64_t* excl_ptr, const int32_t* excl_rows, double lo, double hi,
                            int32_t* position, double* score) {
  return rank_positions_call<fm_batch>(ctx, contexts, candidates, "fm_rank_positions_batch", "fm_rank_positions", tgt_ptr,
                                       tgt_rows, excl_ptr, excl_rows, lo, hi, position, score);
}

int fm_rank_positions_batch_lists(fm_ctx* ctx, fm_batch* contexts, fm_batch* candidates, const fm_lists* tgt,
                                  const fm_lists* excl, double lo, double hi, int32_t* position, double* score) {
  return rank_positions_call<fm_batch>(ctx, contexts, candidates, "fm_rank_positions_batch", "fm_rank_positions", nullptr,
                                       nullptr, nullptr, nullptr, lo, hi, position, score, true, tgt, excl);
}

// ---- resident row lists (fm_lists_*; fm_lists.hip) ----
// what both constructors ask of the context and the sizes
static void lists_args_check(const fm_ctx* ctx, int64_t U, int64_t C, fm_lists** out, const char* call) {
  FM_REQUIRE(out != nullptr, "null out");
  FM_REQUIRE(!ctx->group, std::string(call) + " needs a context of one device: a multi-GPU context's batches are cut over its "
                                              "ranks, and the calls that read resident lists refuse it");
  FM_REQUIRE(U >= 0 && U < (int64_t(1) << 31) && C >= 0 && C < (int64_t(1) << 31),
             "row lists: U and C must be in [0, 2^31), got U = " + std::to_string(U) + ", C = " + std::to_string(C));
}

static std::unique_ptr<fm_lists> new_lists(fm_ctx* ctx, int64_t U, int64_t C) {
  std::unique_ptr<fm_lists> l(new fm_lists());
  l->owner = ctx;
  l->device = ctx->cfg.device;
  l->U = U;
  l->C = C;
  return l;
}

int fm_lists_create(fm_ctx* ctx, int64_t U, int64_t C, const int64_t* ptr, const int32_t* rows, fm_lists** out) {
  return guarded(ctx, [&]() -> int {
    lists_args_check(ctx, U, C, out, "fm_lists_create");
    FM_REQUIRE(ptr != nullptr, "row lists: null ptr");
    const int64_t longest = rank_list_check("row lists: ", "ptr", "rows", ptr, rows, U, C);
    std::unique_ptr<fm_lists> l = new_lists(ctx, U, C);
    l->longest = longest;
    l->host_ptr.assign(ptr, ptr + U + 1);
    const size_t n = (size_t)ptr[U];
    l->ptr.ensure(sizeof(int64_t) * (size_t)(U + 1));
    l->rows.ensure(sizeof(int32_t) * n);
    FM_HIP_CHECK(hipMemcpy(l->ptr.p, ptr, sizeof(int64_t) * (size_t)(U + 1), hipMemcpyHostToDevice));
    if (n) FM_HIP_CHECK(hipMemcpy(l->rows.p, rows, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    *out = l.release();
    return FM_OK;
  });
}

int fm_lists_from_pairs(fm_ctx* ctx, int64_t U, int64_t C, const int32_t* pair_ctx, const int32_t* pair_cand, int64_t n,
                        fm_lists** out) {
  return guarded(ctx, [&]() -> int {
    lists_args_check(ctx, U, C, out, "fm_lists_from_pairs");
    FM_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "n out of range");
    FM_REQUIRE(n == 0 || (pair_ctx != nullptr && pair_cand != nullptr), "null pair lists");
    std::atomic<int> bad{0};
    parallel_chunks(n, int64_t(1) << 18, [&](int64_t lo, int64_t hi) {
      int b = 0;
      for (int64_t i = lo; i < hi; ++i) {
        const int64_t u = pair_ctx[i], c = pair_cand[i];
        b |= (u < 0 || u >= U ? 1 : 0) | (c < 0 || c >= C ? 2 : 0);
      }
      if (b) bad.fetch_or(b);
    });
    FM_REQUIRE(!(bad.load() & 1), "pair_ctx index out of [0, U = " + std::to_string(U) + ")");
    FM_REQUIRE(!(bad.load() & 2), "pair_cand index out of [0, C = " + std::to_string(C) + ")");
    std::unique_ptr<fm_lists> l = new_lists(ctx, U, C);
    l->ptr.ensure(sizeof(int64_t) * (size_t)(U + 1));
    l->host_ptr.assign((size_t)U + 1, 0);
    hipStream_t st = ctx->stream;
    {
      // The call's own scratch, freed where this block ends: the pairs' upload, a sort workspace per sort (a
      // sort's output lies in its workspace, and the context's may be sorting a prepared batch on the side
      // stream), the head flags, their scan.
      DevBuf dctx, dcand, flag, off, ctot, coff, total;
      SortWork by_cand, by_ctx;
      const uint32_t *sctx = nullptr, *scand = nullptr;
      if (n > 0) {
        dctx.ensure(sizeof(int32_t) * (size_t)n);
        dcand.ensure(sizeof(int32_t) * (size_t)n);
        FM_HIP_CHECK(hipMemcpy(dctx.p, pair_ctx, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
        FM_HIP_CHECK(hipMemcpy(dcand.p, pair_cand, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice));
      }
      // (profile "lists_build": the sorts through the compaction, the read-back of the offsets between them included)
      hipEvent_t e0 = ctx->prof_begin(st);
      if (n > 0) {
        // by candidate, then (stable) by context: sorted by (context, candidate)
        const uint32_t *k1 = nullptr, *v1 = nullptr;
        radix_sort_pairs(by_cand, dcand.as<uint32_t>(), dctx.as<uint32_t>(), n, bits_for(C - 1), st, &k1, &v1);
        radix_sort_pairs(by_ctx, v1, k1, n, bits_for(U - 1), st, &sctx, &scand);
      }
      const size_t nchunks = (size_t)std::max<int64_t>(pair_scan_chunks(n), 1);
      flag.ensure(sizeof(uint32_t) * (size_t)std::max<int64_t>(n, 1));
      off.ensure(sizeof(int64_t) * ((size_t)n + 1));
      ctot.ensure(sizeof(int64_t) * nchunks);
      coff.ensure(sizeof(int64_t) * nchunks);
      total.ensure(sizeof(int64_t));
      launch_lists_offsets(sctx, scand, n, U, flag.as<uint32_t>(), off.as<int64_t>(), ctot.as<int64_t>(), coff.as<int64_t>(),
                           total.as<int64_t>(), l->ptr.as<int64_t>(), st);
      // the one read-back: the offsets (the host copy, the longest list, and ptr[U], which sizes rows)
      FM_HIP_CHECK(hipMemcpyAsync(l->host_ptr.data(), l->ptr.p, sizeof(int64_t) * (size_t)(U + 1), hipMemcpyDeviceToHost, st));
      FM_HIP_CHECK(hipStreamSynchronize(st));
      const int64_t rows_n = l->host_ptr[U];
      FM_REQUIRE(rows_n >= 0 && rows_n <= n, "fm_lists_from_pairs: the offsets read back are out of range");
      l->rows.ensure(sizeof(int32_t) * (size_t)rows_n);
      launch_lists_compact(scand, flag.as<uint32_t>(), off.as<int64_t>(), n, l->rows.as<int32_t>(), st);
      ctx->prof_end("lists_build", e0, st);
      FM_HIP_CHECK(hipStreamSynchronize(st));
    }
    for (int64_t u = 0; u < U; ++u) l->longest = std::max(l->longest, l->host_ptr[u + 1] - l->host_ptr[u]);
    *out = l.release();
    return FM_OK;
  });
}

void fm_lists_destroy(fm_lists* l) {
  if (!l) return;
  try {
    delete l;
  } catch (...) {
  }
}

int64_t fm_lists_contexts(const fm_lists* l) { return l ? l->U : -1; }
int64_t fm_lists_candidates(const fm_lists* l) { return l ? l->C : -1; }
int64_t fm_lists_total(const fm_lists* l) { return l ? l->total() : -1; }
int64_t fm_lists_longest(const fm_lists* l) { return l ? l->longest : -1; }

int fm_lists_export(fm_ctx* ctx, const fm_lists* l, int64_t* ptr, int32_t* rows, int64_t cap_rows) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(l != nullptr && l->owner == ctx, "the lists belong to another context");
    const int64_t n = l->total();
    if (ptr) FM_HIP_CHECK(hipMemcpy(ptr, l->ptr.p, sizeof(int64_t) * (size_t)(l->U + 1), hipMemcpyDeviceToHost));
    if (rows) {
      FM_REQUIRE(cap_rows >= n, "cap_rows " + std::to_string(cap_rows) + " is less than the lists' " + std::to_string(n) + " rows");
      if (n) FM_HIP_CHECK(hipMemcpy(rows, l->rows.p, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    }
    return FM_OK;
  });
}

// ---- pair batches (fm_batch_from_pairs / fm_batch_sample_pairs; fm_pairs.hip) ----
// the rules both calls share for their two sources and lists of n pairs
static void pair_args_check(const fm_ctx* ctx, const fm_batch* contexts, const fm_batch* candidates, fm_batch** out,
                            const void* list_a, const void* list_b, int64_t n, const char* call) {
  FM_REQUIRE(out != nullptr && contexts != nullptr && candidates != nullptr, "null argument");
  FM_REQUIRE(contexts->owner == ctx && candidates->owner == ctx, "contexts / candidates belong to another context");
  FM_REQUIRE(n >= 0 && n < (int64_t(1) << 31), "n out of range");
  FM_REQUIRE(n == 0 || (list_a != nullptr && list_b != nullptr), "null pair lists");
  FM_REQUIRE(!ctx->group && !contexts->grp && !candidates->grp,
             std::string(call) + " needs both row sets whole on one device: a multi-GPU context's batches are cut over its "
                                 "ranks (not built from pairs yet)");
  FM_REQUIRE((int64_t)contexts->host_rp.size() == contexts->dev.n_rows + 1 &&
                 (int64_t)candidates->host_rp.size() == candidates->dev.n_rows + 1,
             "contexts and candidates must be batches made by fm_batch_create");
}

// out_batch for two sources
static OutBatch pair_out_batch(fm_ctx* ctx, const fm_batch* contexts, const fm_batch* candidates, fm_batch** out) {
  FM_REQUIRE(*out != contexts && *out != candidates, "out must be a batch of this context other than contexts and candidates");
  return out_batch(ctx, contexts, out, false);
}

// pairs (pc[i], pd[i]), i < n, of two datasets (their host row_ptrs, U and Cn rows) -> rp[n + 1], the row_ptr
// of the concatenated rows, on the pool's threads as selection_row_ptr; 0, or 1 / 2 for an index of pc / pd
// out of range
static int pair_row_ptr(const int64_t* urp, int64_t U, const int64_t* crp, int64_t Cn, const int32_t* pc, const int32_t* pd,
                        int64_t n, int64_t* rp) {
  rp[0] = 0;
  const int64_t T = chunk_count(n, 8192);
  std::vector<int64_t> tot(T + 1, 0);
  std::atomic<int> bad{0};
  parallel_chunks_t(n, T, [&](int64_t t, int64_t lo, int64_t hi) {
    int64_t acc = 0;
    for (int64_t i = lo; i < hi; ++i) {
      const int64_t u = pc[i], c = pd[i];
      if (u < 0 || u >= U || c < 0 || c >= Cn) {
        bad.fetch_or(u < 0 || u >= U ? 1 : 2);
        return;
      }
      acc += (urp[u + 1] - urp[u]) + (crp[c + 1] - crp[c]);
      rp[i + 1] = acc;
    }
    tot[t + 1] = acc;
  });
  if (bad.load()) return (bad.load() & 1) ? 1 : 2;
  for (int64_t t = 0; t < T; ++t) tot[t + 1] += tot[t];  // the chunks' offsets
  if (T > 1)
    parallel_chunks_t(n, T, [&](int64_t t, int64_t lo, int64_t hi) {
      const int64_t add = tot[t];
      if (add)
        for (int64_t i = lo; i < hi; ++i) rp[i + 1] += add;
    });
  return 0;
}

// b is about to be refilled on the copy stream (as fm_batch_from_rows refills its result): a split view
// detached, the events made, and the stream waiting for every queued read of the batch
static hipStream_t pair_refill_begin(fm_ctx* ctx, fm_batch* b) {
  b->detach_view();
  b->ensure_events(ctx->stream);
  // (sel_copied is recorded only behind a staging copy, on the copy stream: fm_batch_sample_pairs stages
  // nothing in the batch, and a wait for an event never recorded returns at once)
  if (!b->built) {
    FM_HIP_CHECK(hipEventCreateWithFlags(&b->built, hipEventDisableTiming));
    FM_HIP_CHECK(hipEventCreateWithFlags(&b->sel_copied, hipEventDisableTiming));
  }
  if (!ctx->copy_stream) FM_HIP_CHECK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
  hipStream_t gs = ctx->copy_stream;
  FM_HIP_CHECK(hipStreamWaitEvent(gs, b->last_use, 0));
  if (b->sh && b->sh->last_use) FM_HIP_CHECK(hipStreamWaitEvent(gs, b->sh->last_use, 0));
  if (b->prepared && b->ready) FM_HIP_CHECK(hipStreamWaitEvent(gs, b->ready, 0));
  return gs;
}

static void pair_refill_end(fm_batch* b, const fm_batch* contexts, const fm_batch* candidates, hipStream_t gs) {
  FM_HIP_CHECK(hipEventRecord(b->built, gs));
  b->max_id = std::max(contexts->max_id, candidates->max_id);
  b->prepared = false;  // a refilled batch is sorted again by its own fm_batch_prepare
  b->host_rp.clear();   // not itself a dataset
}

int fm_batch_from_pairs(fm_ctx* ctx, const fm_batch* contexts, const fm_batch* candidates, const int32_t* pair_ctx,
                        const int32_t* pair_cand, const double* label, int64_t n, fm_batch** out) {
  return guarded(ctx, [&]() -> int {
    pair_args_check(ctx, contexts, candidates, out, pair_ctx, pair_cand, n, "fm_batch_from_pairs");
    FM_REQUIRE(n == 0 || label != nullptr, "null label");
    OutBatch res = pair_out_batch(ctx, contexts, candidates, out);
    fm_batch* b = res.b;
    // the staging of this batch's previous selection has been copied out
    if (b->sel_copied) FM_HIP_CHECK(hipEventSynchronize(b->sel_copied));
    // staging {row_ptr int64 [n + 1], label double [n], pair_ctx int32 [n], pair_cand int32 [n]}: the result's
    // row_ptr straight into it from the two datasets' host row_ptrs (the indices validated on the way)
    const size_t img = sizeof(int64_t) * ((size_t)n + 1) + sizeof(double) * (size_t)n + 2 * sizeof(int32_t) * (size_t)n;
    b->sel_pin.ensure_slack(img);
    int64_t* rp = reinterpret_cast<int64_t*>(b->sel_pin.p);
    double* hl = reinterpret_cast<double*>(rp + n + 1);
    int32_t* hc = reinterpret_cast<int32_t*>(hl + n);
    int32_t* hd = hc + n;
    const int bad = pair_row_ptr(contexts->host_rp.data(), contexts->dev.n_rows, candidates->host_rp.data(),
                                 candidates->dev.n_rows, pair_ctx, pair_cand, n, rp);
    FM_REQUIRE(bad != 1, "pair_ctx index out of [0, rows of contexts)");
    FM_REQUIRE(bad != 2, "pair_cand index out of [0, rows of candidates)");
    const int64_t N = rp[n];
    FM_REQUIRE(N < (int64_t(1) << 31), "nnz must be < 2^31 per batch");
    if (n > 0) {
      std::memcpy(hl, label, sizeof(double) * (size_t)n);
      std::memcpy(hc, pair_ctx, sizeof(int32_t) * (size_t)n);
      std::memcpy(hd, pair_cand, sizeof(int32_t) * (size_t)n);
    }
    // batch-only work on the copy stream, behind every queued read of the batch (fm_batch_from_rows)
    hipStream_t gs = pair_refill_begin(ctx, b);
    size_batch(b->dev, n, N);
    b->up.ensure_slack(img + 16);
    FM_HIP_CHECK(hipMemcpyAsync(b->up.p, b->sel_pin.p, img, hipMemcpyHostToDevice, gs));
    FM_HIP_CHECK(hipEventRecord(b->sel_copied, gs));
    const int64_t* drp = b->up.as<int64_t>();
    hipEvent_t e0 = ctx->prof_begin(gs);
    if (n > 0) {
      const double* dl = reinterpret_cast<const double*>(drp + n + 1);
      const int32_t* dc = reinterpret_cast<const int32_t*>(dl + n);
      launch_pair_rows(dc, dc + n, drp, dl, contexts->dev, candidates->dev, n, b->dev, gs);
    } else {
      FM_HIP_CHECK(hipMemcpyAsync(b->dev.row_ptr.p, drp, sizeof(int64_t), hipMemcpyDeviceToDevice, gs));
    }
    ctx->prof_end("pair_gather", e0, gs);
    pair_refill_end(b, contexts, candidates, gs);
    b->row_group = 0;
    res.commit();
    return FM_OK;
  });
}

// Both forms of the sampled call: the exclude lists as host arrays (excl_ptr / excl_rows: checked, staged and
// uploaded with the positives) or -- resident -- as an fm_lists (rex; null: none), whose device buffers the
// draw reads where they are: only the positives are staged, and the E >= 1 rule reads the object's host offsets.
static int sample_pairs_call(fm_ctx* ctx, const fm_batch* contexts, const fm_batch* candidates, const int32_t* pos_ctx,
                             const int32_t* pos_cand, int64_t n_pos, int32_t n_neg, const int64_t* excl_ptr,
                             const int32_t* excl_rows, bool resident, const fm_lists* rex, double pos_label, double neg_label,
                             uint64_t seed, fm_batch** out, int32_t* sampled) {
  return guarded(ctx, [&]() -> int {
    pair_args_check(ctx, contexts, candidates, out, pos_ctx, pos_cand, n_pos, "fm_batch_sample_pairs");
    FM_REQUIRE(n_neg >= 0 && n_neg <= 1024, "n_neg must be in [0, 1024], got " + std::to_string(n_neg));
    const int64_t per = (int64_t)n_neg + 1, B = n_pos * per;
    FM_REQUIRE(B < (int64_t(1) << 31), "n_pos * (1 + n_neg) must be < 2^31");
    const int64_t U = contexts->dev.n_rows, Cn = candidates->dev.n_rows;
    FM_REQUIRE(Cn < (int64_t(1) << 31) && U < (int64_t(1) << 31), "fewer than 2^31 rows per source");
    // (profile: the host phases of the lists beside the device phases, tools/pair_bench.py)
    const auto host_ms = [](std::chrono::steady_clock::time_point t0) {
      return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    auto t0 = std::chrono::steady_clock::now();
    RankList ex;
    if (resident && rex) ex = resident_list(ctx, rex, U, Cn, "excl");
    else if (excl_ptr) ex = {excl_ptr, excl_rows, rank_list_check("exclude list: ", "excl_ptr", "excl_rows", excl_ptr, excl_rows, U, Cn)};
    if (ex.dev_ptr) excl_ptr = nullptr;  // (resident: from here on the host arrays are the positives alone)
    ctx->prof_host("pair_lists_check", host_ms(t0));
    for (int64_t i = 0; i < n_pos; ++i) {
      const int64_t u = pos_ctx[i], c = pos_cand[i];
      FM_REQUIRE(u >= 0 && u < U, "pos_ctx index out of [0, rows of contexts)");
      FM_REQUIRE(c >= 0 && c < Cn, "pos_cand index out of [0, rows of candidates)");
      const int64_t L = ex.ptr ? ex.ptr[u + 1] - ex.ptr[u] : 0;
      FM_REQUIRE(Cn - L >= 1, "context " + std::to_string(u) + " (positive " + std::to_string(i) +
                                  ") has no eligible candidate row: its exclude list holds every row");
    }
    OutBatch res = pair_out_batch(ctx, contexts, candidates, out);
    fm_batch* b = res.b;
    // The draw, the lengths, the scan and the read-back of the entry count run in the context's scratch on
    // the copy stream before *out is touched or waited for: the one host wait of this call is for them (and
    // for what the copy stream held before: earlier gathers), never for the main or the side stream.
    if (!ctx->copy_stream) FM_HIP_CHECK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    hipStream_t gs = ctx->copy_stream;
    PairWork& w = ctx->pairs;
    const size_t n_ex = excl_ptr ? (size_t)excl_ptr[U] : 0;
    // staging: {total int64, pad} | excl_ptr int64 [U + 1] | pos_ctx, pos_cand int32 [n_pos] | excl_rows int32 [n_ex]
    // | the drawn pairs' candidate rows int32 [B] on their way back (sampled != NULL)
    const size_t o_ptr = 16, o_pc = o_ptr + sizeof(int64_t) * (excl_ptr ? (size_t)U + 1 : 0);
    const size_t o_pd = o_pc + sizeof(int32_t) * (size_t)n_pos, o_ex = o_pd + sizeof(int32_t) * (size_t)n_pos;
    const size_t o_back = (o_ex + sizeof(int32_t) * n_ex + 15) / 16 * 16;
    const size_t lists_bytes = o_back - o_ptr;
    ctx->pair_pin.ensure_slack(o_back + (sampled ? sizeof(int32_t) * (size_t)B : 0));
    char* pin = reinterpret_cast<char*>(ctx->pair_pin.p);
    t0 = std::chrono::steady_clock::now();
    if (excl_ptr) std::memcpy(pin + o_ptr, excl_ptr, sizeof(int64_t) * ((size_t)U + 1));
    if (n_pos > 0) {
      std::memcpy(pin + o_pc, pos_ctx, sizeof(int32_t) * (size_t)n_pos);
      std::memcpy(pin + o_pd, pos_cand, sizeof(int32_t) * (size_t)n_pos);
    }
    if (n_ex)
      parallel_chunks((int64_t)n_ex, 1 << 20, [&](int64_t lo, int64_t hi) {
        std::memcpy(pin + o_ex + sizeof(int32_t) * (size_t)lo, excl_rows + lo, sizeof(int32_t) * (size_t)(hi - lo));
      });
    ctx->prof_host("pair_lists_stage", host_ms(t0));
    const size_t rows = (size_t)std::max<int64_t>(B, 1);
    const size_t nchunks = (size_t)std::max<int64_t>(pair_scan_chunks(B), 1);
    w.lists.ensure_slack(lists_bytes + 16);
    w.pair_ctx.ensure_slack(sizeof(int32_t) * rows);
    w.pair_cand.ensure_slack(sizeof(int32_t) * rows);
    w.label.ensure_slack(sizeof(double) * rows);
    w.len.ensure_slack(sizeof(uint32_t) * rows);
    w.row_ptr.ensure_slack(sizeof(int64_t) * (rows + 1));
    w.chunk_tot.ensure_slack(sizeof(int64_t) * nchunks);
    w.chunk_off.ensure_slack(sizeof(int64_t) * nchunks);
    w.total.ensure(sizeof(int64_t));
    hipEvent_t e0 = ctx->prof_begin(gs);
    if (lists_bytes) FM_HIP_CHECK(hipMemcpyAsync(w.lists.p, pin + o_ptr, lists_bytes, hipMemcpyHostToDevice, gs));
    ctx->prof_end("pair_lists_upload", e0, gs);
    e0 = ctx->prof_begin(gs);
    const char* dl = w.lists.as<char>();  // the staging from o_ptr on
    launch_pair_sample(reinterpret_cast<const int32_t*>(dl + (o_pc - o_ptr)), reinterpret_cast<const int32_t*>(dl + (o_pd - o_ptr)),
                       n_pos, n_neg, ex.dev_ptr ? ex.dev_ptr : excl_ptr ? reinterpret_cast<const int64_t*>(dl) : nullptr,
                       ex.dev_ptr ? ex.dev_rows : reinterpret_cast<const int32_t*>(dl + (o_ex - o_ptr)), pos_label, neg_label, seed,
                       contexts->dev,
                       candidates->dev,
                       w.pair_ctx.as<int32_t>(), w.pair_cand.as<int32_t>(), w.label.as<double>(), w.len.as<uint32_t>(),
                       w.row_ptr.as<int64_t>(), w.chunk_tot.as<int64_t>(), w.chunk_off.as<int64_t>(), w.total.as<int64_t>(),
                       gs);
    ctx->prof_end("pair_draw", e0, gs);
    FM_HIP_CHECK(hipMemcpyAsync(pin, w.total.p, sizeof(int64_t), hipMemcpyDeviceToHost, gs));
    if (sampled && B > 0)
      FM_HIP_CHECK(hipMemcpyAsync(pin + o_back, w.pair_cand.p, sizeof(int32_t) * (size_t)B, hipMemcpyDeviceToHost, gs));
    FM_HIP_CHECK(hipStreamSynchronize(gs));
    const int64_t N = *reinterpret_cast<const int64_t*>(pin);
    FM_REQUIRE(N < (int64_t(1) << 31), "nnz must be < 2^31 per batch");
    if (sampled) {
      const int32_t* back = reinterpret_cast<const int32_t*>(pin + o_back);
      for (int64_t i = 0; i < n_pos; ++i)
        for (int64_t j = 0; j < n_neg; ++j) sampled[i * n_neg + j] = back[i * per + 1 + j];
    }
    // only now is *out sized and refilled, behind every queued read of it (fm_batch_from_rows)
    gs = pair_refill_begin(ctx, b);
    size_batch(b->dev, B, N);
    e0 = ctx->prof_begin(gs);
    if (B > 0)
      launch_pair_rows(w.pair_ctx.as<int32_t>(), w.pair_cand.as<int32_t>(), w.row_ptr.as<int64_t>(), w.label.as<double>(),
                       contexts->dev, candidates->dev, B, b->dev, gs);
    else
      FM_HIP_CHECK(hipMemcpyAsync(b->dev.row_ptr.p, w.row_ptr.p, sizeof(int64_t), hipMemcpyDeviceToDevice, gs));
    ctx->prof_end("pair_gather", e0, gs);
    pair_refill_end(b, contexts, candidates, gs);
    b->row_group = n_neg >= 1 ? (int32_t)per : 0;  // a positive and its negatives; none: ungrouped
    res.commit();
    return FM_OK;
  });
}

int fm_batch_sample_pairs(fm_ctx* ctx, const fm_batch* contexts, const fm_batch* candidates, const int32_t* pos_ctx,
                          const int32_t* pos_cand, int64_t n_pos, int32_t n_neg, const int64_t* excl_ptr,
                          const int32_t* excl_rows, double pos_label, double neg_label, uint64_t seed, fm_batch** out,
                          int32_t* sampled) {
  return sample_pairs_call(ctx, contexts, candidates, pos_ctx, pos_cand, n_pos, n_neg, excl_ptr, excl_rows, false, nullptr,
                           pos_label, neg_label, seed, out, sampled);
}

int fm_batch_sample_pairs_lists(fm_ctx* ctx, const fm_batch* contexts, const fm_batch* candidates, const int32_t* pos_ctx,
                                const int32_t* pos_cand, int64_t n_pos, int32_t n_neg, const fm_lists* excl, double pos_label,
                                double neg_label, uint64_t seed, fm_batch** out, int32_t* sampled) {
  return sample_pairs_call(ctx, contexts, candidates, pos_ctx, pos_cand, n_pos, n_neg, nullptr, nullptr, true, excl, pos_label,
                           neg_label, seed, out, sampled);
}

int fm_init_from_batch(fm_ctx* ctx, fm_batch* b, int64_t* n_present) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(b != nullptr && b->owner == ctx, "batch belongs to another context");
    if (ctx->group) return group_init_from_batch(ctx, b, n_present);
    wait_built(b, ctx->stream);
    launch_init_entries(ctx->view(), b->dev.col.as<uint32_t>(), b->dev.nnz, ctx->cfg.seed, ctx->cfg.init_sd, ctx->epoch,
                        ctx->cum_host.back(), ctx->stream);
    if (n_present) {
      DevBuf d;
      d.ensure(sizeof(int64_t));
      launch_count_present(ctx->view(), d.as<int64_t>(), ctx->stream);
      FM_HIP_CHECK(hipMemcpyAsync(n_present, d.p, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
      FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    } else {
      FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    }
    return FM_OK;
  });
}

static int loss_grad_impl(fm_ctx* ctx, const fm_csr* csr, double fill_sd, uint64_t seed, double* pred, double* loss,
                          double* dw, double* dv) {
  if (ctx && ctx->group) {
    // a replicated group's replicas are identical: member 0 answers, with the group locked so that
    // no group step is caught between a member's fm_repl_grad and fm_repl_apply
    return guarded(ctx, [&]() -> int {
      FM_REQUIRE(ctx->cfg.parallel == FM_PARALLEL_REPLICATED,
                 "fm_loss_grad needs the whole table (a replicated or single-table context)");
      return loss_grad_impl(group_member0(ctx), csr, fill_sd, seed, pred, loss, dw, dv);
    });
  }
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(ctx->cfg.shard_count == 1, "fm_loss_grad needs the whole table (shard_count == 1)");
    FM_REQUIRE(csr != nullptr, "null argument");
    if (csr->n_rows == 0 || csr->nnz == 0) return FM_OK;
    fm_batch* b = host_batch(ctx);
    // the fill covers ids the table cannot hold too (ids >= num_features, the left outer join)
    upload_batch(ctx, csr, b, fill_sd <= 0.0);
    const int64_t N = csr->nnz;
    const int k = ctx->cfg.k;
    DevBuf dpred, dloss, ddw, ddv, dabs;
    dpred.ensure(sizeof(double) * N);
    dloss.ensure(sizeof(double) * N);
    ddw.ensure(sizeof(double) * N);
    ddv.ensure(sizeof(double) * N * k);
    dabs.ensure(sizeof(int32_t));
    FM_HIP_CHECK(hipMemsetAsync(dabs.p, 0, sizeof(int32_t), ctx->stream));
    launch_loss_grad(ctx->view(), b->dev, ctx->cum_host.back(), ctx->cfg.w0, dpred.as<double>(), dloss.as<double>(),
                     ddw.as<double>(), ddv.as<double>(), dabs.as<int32_t>(), ctx->stream, fill_sd, seed);
    int32_t absent = 0;
    FM_HIP_CHECK(hipMemcpyAsync(&absent, dabs.p, sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    FM_REQUIRE(fill_sd > 0.0 || absent == 0, "batch references feature ids absent from the model");
    if (pred) FM_HIP_CHECK(hipMemcpy(pred, dpred.p, sizeof(double) * N, hipMemcpyDeviceToHost));
    if (loss) FM_HIP_CHECK(hipMemcpy(loss, dloss.p, sizeof(double) * N, hipMemcpyDeviceToHost));
    if (dw) FM_HIP_CHECK(hipMemcpy(dw, ddw.p, sizeof(double) * N, hipMemcpyDeviceToHost));
    if (dv) FM_HIP_CHECK(hipMemcpy(dv, ddv.p, sizeof(double) * N * k, hipMemcpyDeviceToHost));
    return FM_OK;
  });
}

int fm_loss_grad(fm_ctx* ctx, const fm_csr* csr, double* pred, double* loss, double* dw, double* dv) {
  return loss_grad_impl(ctx, csr, 0.0, 0, pred, loss, dw, dv);
}

int fm_calc_loss_grad(fm_ctx* ctx, const fm_csr* csr, double initial_sd, uint64_t seed, double* pred, double* loss,
                      double* dw, double* dv) {
  if (!(initial_sd > 0.0) || !std::isfinite(initial_sd)) {
    set_error("requirement failed: initSd (initial Standard Deviation) must be > 0.0");
    return FM_ERR_ARG;
  }
  return loss_grad_impl(ctx, csr, initial_sd, seed, pred, loss, dw, dv);
}

int fm_vector_sum_by_key(fm_ctx* ctx, const int32_t* keys, int64_t n, const double* vecs, int32_t k,
                         int32_t* out_keys, double* out_sums, int64_t* n_out) {
  if (ctx && ctx->group)  // on member 0's device, with the group locked
    return guarded(ctx, [&]() -> int {
      return fm_vector_sum_by_key(group_member0(ctx), keys, n, vecs, k, out_keys, out_sums, n_out);
    });
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(n >= 0 && k >= 1 && n_out, "bad arguments");
    *n_out = 0;
    if (n == 0) return FM_OK;
    FM_REQUIRE(keys && vecs && out_keys && out_sums, "null argument");
    int64_t mx = 0;
    for (int64_t i = 0; i < n; ++i) {
      FM_REQUIRE(keys[i] >= 0, "negative key");
      mx = std::max<int64_t>(mx, keys[i]);
    }
    DevBuf dk, dvec, dok, dos, drun, dn;
    SortWork sw;
    dk.ensure(sizeof(uint32_t) * n);
    dvec.ensure(sizeof(double) * n * k);
    dok.ensure(sizeof(int32_t) * n);
    dos.ensure(sizeof(double) * n * k);
    drun.ensure(sizeof(uint32_t) * n);
    dn.ensure(sizeof(int64_t));
    FM_HIP_CHECK(hipMemcpy(dk.p, keys, sizeof(int32_t) * n, hipMemcpyHostToDevice));
    FM_HIP_CHECK(hipMemcpy(dvec.p, vecs, sizeof(double) * n * k, hipMemcpyHostToDevice));
    const uint32_t *sk = nullptr, *sv = nullptr;
    radix_sort_pairs(sw, dk.as<uint32_t>(), nullptr, n, bits_for(mx), ctx->stream, &sk, &sv);
    launch_segment_sum(sk, sv, n, dvec.as<double>(), k, drun.as<uint32_t>(), dok.as<int32_t>(), dos.as<double>(),
                       dn.as<int64_t>(), ctx->stream);
    int64_t nu = 0;
    FM_HIP_CHECK(hipMemcpyAsync(&nu, dn.p, sizeof(int64_t), hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    FM_HIP_CHECK(hipMemcpy(out_keys, dok.p, sizeof(int32_t) * nu, hipMemcpyDeviceToHost));
    FM_HIP_CHECK(hipMemcpy(out_sums, dos.p, sizeof(double) * nu * k, hipMemcpyDeviceToHost));
    *n_out = nu;
    return FM_OK;
  });
}

int fm_profile_enable(fm_ctx* ctx, int32_t on) {
  return guarded(ctx, [&]() -> int {
    if (ctx->group) return group_profile(ctx, 0, on, nullptr, 0, nullptr, nullptr, 0, nullptr);
    ctx->prof = on != 0;
    return FM_OK;
  });
}

int fm_profile_reset(fm_ctx* ctx) {
  return guarded(ctx, [&]() -> int {
    if (ctx->group) return group_profile(ctx, 1, 0, nullptr, 0, nullptr, nullptr, 0, nullptr);
    ctx->resolve_profile();
    ctx->prof_acc.clear();
    ctx->prof_order.clear();
    return FM_OK;
  });
}

int fm_profile_read(fm_ctx* ctx, char* names, int64_t names_cap, double* total_ms, int64_t* launches, int64_t cap,
                    int64_t* n) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(n != nullptr, "null n");
    if (ctx->group) return group_profile(ctx, 2, 0, names, names_cap, total_ms, launches, cap, n);
    ctx->resolve_profile();
    *n = (int64_t)ctx->prof_order.size();
    std::string joined;
    int64_t i = 0;
    for (const auto& nm : ctx->prof_order) {
      if (i < cap) {
        if (total_ms) total_ms[i] = ctx->prof_acc[nm].ms;
        if (launches) launches[i] = ctx->prof_acc[nm].n;
      }
      if (!joined.empty()) joined += "\n";
      joined += nm;
      ++i;
    }
    if (names && names_cap > 0) {
      const size_t m = std::min<size_t>((size_t)names_cap - 1, joined.size());
      std::memcpy(names, joined.data(), m);
      names[m] = '\0';
    }
    return FM_OK;
  });
}

int fm_repl_grad(fm_ctx* ctx, fm_batch* batch, void* grad) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(!ctx->group, "a multi-GPU context runs its replicated step itself (fm_step / fm_step_batch)");
    require_squared(ctx, "fm_repl_grad");
    FM_REQUIRE(grad != nullptr, "null gradient buffer");
    FM_REQUIRE(!ctx->repl_pending, "fm_repl_apply must follow fm_repl_grad");
    ctx->ensure_hist(ctx->epoch + 1);
    double* stats = ctx->loss_hist.as<double>() + 3 * (int64_t)ctx->epoch;
    FM_HIP_CHECK(hipMemsetAsync(stats, 0, sizeof(double) * 3, ctx->stream));
    const int rc = step_impl(ctx, batch, 1, 0.0, 0.0, nullptr, reinterpret_cast<float*>(grad));
    ctx->repl_pending = true;
    return rc;
  });
}

int fm_repl_apply(fm_ctx* ctx, const void* grad, int32_t t, double step_size, double reg_param,
                  int64_t global_rows) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(!ctx->group, "a multi-GPU context runs its replicated step itself (fm_step / fm_step_batch)");
    require_squared(ctx, "fm_repl_apply");
    FM_REQUIRE(ctx->repl_pending, "fm_repl_grad must run first");
    FM_REQUIRE(global_rows >= 0, "negative global_rows");
    ctx->repl_pending = false;
    if (global_rows == 0) return FM_NOTHING_TO_DO;  // SGD.scala:126-128 (every rank skips)
    FM_REQUIRE(grad != nullptr, "null gradient buffer");
    FM_REQUIRE(t >= 1, "iteration index t must be >= 1");
    FM_REQUIRE(std::isfinite(step_size) && std::isfinite(reg_param), "non-finite step size / regParam");
    StepParams p{};
    p.n_rows = global_rows;
    p.eta = step_size / std::sqrt((double)t);  // SGD.scala:121
    p.lam = p.eta * reg_param;                 // SGD.scala:122
    p.m = (double)global_rows;                 // global miniBatchSize
    p.scale_v = p.eta / (double)global_rows;
    p.epoch = ctx->epoch;
    p.cumE = ctx->cum_host.back();
    p.cum_next = p.cumE + p.lam;
    p.w0 = ctx->cfg.w0;
    ctx->ensure_hist(ctx->epoch + 1);
    ctx->repl_cnt.ensure(sizeof(uint32_t) * kReplApplyBlocks);
    hipEvent_t e0 = ctx->prof_begin(ctx->stream);
    double* stats = ctx->loss_hist.as<double>() + 3 * (int64_t)ctx->epoch;
    launch_repl_apply(ctx->view(), reinterpret_cast<const float*>(grad), p, ctx->repl_cnt.as<uint32_t>(), stats + 2,
                      ctx->stream);
    ctx->prof_end("apply", e0, ctx->stream);
    ctx->epoch += 1;
    ctx->cum_host.push_back(p.cum_next);
    return FM_OK;
  });
}

int fm_last_stats(fm_ctx* ctx, double* loss_sum, int64_t* n_loss_rows, int64_t* n_unique) {
  return guarded(ctx, [&]() -> int {
    FM_REQUIRE(loss_sum && n_loss_rows && n_unique, "null argument");
    if (ctx->group) return group_last_stats(ctx, loss_sum, n_loss_rows, n_unique);
    FM_REQUIRE(ctx->epoch >= 1, "no step executed");
    double h[3];
    FM_HIP_CHECK(hipMemcpyAsync(h, ctx->loss_hist.as<double>() + 3 * (int64_t)(ctx->epoch - 1), sizeof(h),
                                hipMemcpyDeviceToHost, ctx->stream));
    FM_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *loss_sum = h[0];
    *n_loss_rows = (int64_t)h[1];
    *n_unique = (int64_t)h[2];
    return FM_OK;
  });
}

}  // extern "C"
