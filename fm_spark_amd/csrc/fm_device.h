// Device helpers shared by the step kernels (fm_forward.hip, fm_update.hip, fm_table.hip,
// fm_batch.hip) and the sharded / grouped paths (fm_shard.hip, fm_group.hip): every piece of the
// row arithmetic that more than one kernel performs is defined here, once.
//
// One iteration of FactorizationMachinesSGD.runMiniBatchSGD's fold body
// (FactorizationMachinesSGD.scala:116-211) is, on the device:
//
//   k_forward          (fm_forward.hip) sample-major.  A team of TEAM lanes owns one sample; GS lanes
//                      hold one k-wide V row as float4 quads (coalesced 16 B per lane), so a pass covers
//                      TEAM/GS of the sample's entries; four passes are issued before any is
//                      consumed.  Pending L1 is applied on the fly (lazy soft-threshold, below).
//                      fp64 accumulation of vfxiSum (S), the linear and v^2 x^2 terms, yhat and
//                      the loss partial (FactorizationMachinesModel.scala:173-233).
//   radix sort         (fm_sort.hip) entries by feature slot -> CSC order, stable; runs on a
//                      second stream concurrently with k_forward (it only reads the batch).
//   k_segment_update   (fm_update.hip) feature-major.  One wave per 64 sorted entries, one lane per
//                      entry: per-entry gradient (SGD.scala:145-146, keeping the reference's
//                      x*yhat - y w-gradient), fixed-order segmented scan across lanes, and
//                      the tail lane of every complete run applies the fused update + L1
//                      (SGD.scala:150-181) to its row.  Runs that cross a 64-entry chunk write
//                      fp64 partials instead.
//   k_segment_combine  (fm_update.hip) one wave per crossing run sums its partials in chunk order
//                      (lanes over the k+1 columns) and applies the same update; block 0 closes the
//                      step (loss sum and distinct-id count, fixed-order reductions).
//
// Lazy L1.  The reference soft-thresholds EVERY model row every iteration (outer joins,
// SGD.scala:157-181).  S_b(S_a(z)) = S_{a+b}(z) for a, b >= 0, so each row header keeps the
// cumulative shrink `cum` it has received; a row read when the running total is cumE is first
// brought current by S_{cumE - cum}.  Export flushes every row.
#pragma once

#include "fm_internal.h"

namespace fmhip {

// Plain cached loads and stores throughout: nontemporal variants of the row write-back, the sorted
// entry stream, the CSR stream and the sort's streams were measured (round 2) and
// were neutral or slower in the step.

constexpr int kBlock = 256;  // threads per block of the step, table and batch kernels

inline unsigned grid_for(int64_t n, int block, int64_t cap = 256 * 16) {
  int64_t g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (unsigned)g;
}

// Block barrier that orders LDS only: the waits it implies are lgkmcnt, not vmcnt, so global
// loads issued ahead and global stores still draining stay in flight across it (__syncthreads'
// workgroup fence waits for every outstanding global access of the wave).
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// The lanes of one wave hand LDS contents to each other: what they wrote before, all see after.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Deterministic block reduction of the per-thread loss partials {sum of squared errors, rows
// counted} into loss_part[blockIdx.x]: xor tree within each wave, then the waves in order.
__device__ __forceinline__ void block_loss_partial(double loss_acc, double nloss, double2* __restrict__ loss_part) {
  const int tid = threadIdx.x;
  __shared__ double red[2][kBlock / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    loss_acc += __shfl_xor(loss_acc, o);
    nloss += __shfl_xor(nloss, o);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = loss_acc;
    red[1][tid >> 6] = nloss;
  }
  __syncthreads();
  if (tid == 0) {
    double l = 0.0, c = 0.0;
    for (int w = 0; w < kBlock / 64; ++w) {
      l += red[0][w];
      c += red[1][w];
    }
    loss_part[blockIdx.x] = make_double2(l, c);
  }
}

// Evaluation (kEvaluate, k_shard_evaluate, k_eval_fold): a thread's record of the rows it scored,
// kEvalRec fp64 sums {rows, rows without a learned entry, sum e, sum |e|, sum e^2} of e = label -
// prediction.  (The counts are sums of 1.0: exact below 2^53 rows.)
struct EvalAcc {
  double v[kEvalRec] = {0.0, 0.0, 0.0, 0.0, 0.0};
};
// One row into the record: the prediction is FactorizationMachinesModel.predict's (Model.scala:86,
// :129-132: w0 unclamped for a row without a learned entry, else the clamped yhat); returns it, so
// that what a caller stores is the value that was subtracted.
__device__ __forceinline__ double eval_row(EvalAcc& a, double yhat, bool learned, double w0, double lo, double hi,
                                           double y) {
  const double p = learned ? fmin(fmax(yhat, lo), hi) : w0;
  const double e = y - p;
  a.v[0] += 1.0;
  a.v[1] += learned ? 0.0 : 1.0;
  a.v[2] += e;
  a.v[3] += fabs(e);
  a.v[4] += e * e;
  return p;
}
// block_loss_partial's reduction for the record: each sum through the xor tree within a wave, then
// the waves in order, into out[kEvalRec] (thread 0).  The order depends on the block shape alone.
__device__ __forceinline__ void block_eval_partial(EvalAcc a, double* __restrict__ out) {
  const int tid = threadIdx.x;
  __shared__ double red[kEvalRec][kBlock / 64];
#pragma unroll
  for (int i = 0; i < kEvalRec; ++i) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) a.v[i] += __shfl_xor(a.v[i], o);
    if ((tid & 63) == 0) red[i][tid >> 6] = a.v[i];
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < kEvalRec; ++i) {
      double s = 0.0;
      for (int w = 0; w < kBlock / 64; ++w) s += red[i][w];
      out[i] = s;
    }
  }
}

// The logistic forms of the objective stage (fm_objective.hip) and the binary evaluation (fm_binary.hip),
// fp64 and finite for every finite z:
//   sigma(z) = 1 / (1 + e) or e / (1 + e), e = exp(-|z|);   softplus(z) = max(z, 0) + log1p(exp(-|z|)).
__device__ __forceinline__ double sigmoid_d(double z) {
  const double e = exp(-fabs(z));  // in (0, 1]
  const double s = 1.0 / (1.0 + e);
  return z >= 0.0 ? s : e * s;
}
__device__ __forceinline__ double softplus_d(double z) { return fmax(z, 0.0) + log1p(exp(-fabs(z))); }

__device__ __forceinline__ void st_row4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

__device__ __forceinline__ float shrink_f(float z, double a) {
  // signum(z) * max(0, |z| - a) (FactorizationMachinesSGD.scala:104, :179), in fp64.
  const double az = fabs((double)z) - a;
  return az > 0.0 ? (float)copysign(az, (double)z) : 0.0f * z;
}

__device__ __forceinline__ double shrink_d(double z, double a) {
  const double az = fabs(z) - a;
  return az > 0.0 ? copysign(az, z) : 0.0 * z;
}

__device__ __forceinline__ float4 shrink4(float4 v, double a) {
  return make_float4(shrink_f(v.x, a), shrink_f(v.y, a), shrink_f(v.z, a), shrink_f(v.w, a));
}

// fp32 soft-threshold, for the row catch-up and the update's final rounding: the operands are
// fp32 values and fp32-rounded shrink amounts, the result differs from the fp64 form by at most
// one rounding of the fp32 result.
__device__ __forceinline__ float shrink1f(float z, float a) { return copysignf(fmaxf(fabsf(z) - a, 0.f), z); }
__device__ __forceinline__ float4 shrink4f(float4 v, float a) {
  return make_float4(shrink1f(v.x, a), shrink1f(v.y, a), shrink1f(v.z, a), shrink1f(v.w, a));
}

// The row header and one V quad brought current (absent rows read as zero).
__device__ __forceinline__ void current_row(const RowHdr& h, float4& v, float& w, double cumE) {
  if (h.t < 0) {
    w = 0.f;
    v = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  w = h.w;
  const double a = cumE - h.cum;
  if (a > 0.0) {
    w = shrink_f(w, a);
    v = shrink4(v, a);
  }
}

// Inclusive segmented scan over lanes [start_lane, lane] in a fixed tree order.  nsteps is the
// wave-uniform depth the longest piece needs; the skipped steps would add nothing, so the
// result is bitwise that of the full 6-step scan.
__device__ __forceinline__ double seg_scan(double v, int lane, int start_lane, int nsteps) {
  for (int i = 0; i < nsteps; ++i) {
    const int o = 1 << i;
    const double t = __shfl_up(v, o);
    if (lane - o >= start_lane) v += t;
  }
  return v;
}

// Floats of the row header and the zero pad after it, to the end of the 64-B memory granule that
// holds the header.
__device__ __forceinline__ int hdr_span(int kp) { return 4 + ((16 - ((kp + 4) & 15)) & 15); }

// Header store that completes the 64-B memory granule holding it: the header, then zero
// padding to the granule's end.  A partly written granule costs a read-modify-write in HBM
// (measured on MI355X, tools/traffic_cal.hip: random 80-B row writes 0.58 ms per 10M rows, the
// same rows written as whole 128-B lines 0.37 ms); the V quads that share the granule are
// written by the same kernel, so the granule leaves L2 whole.
__device__ __forceinline__ void store_hdr(const TableView& T, int64_t slot, const RowHdr& o) {
  float* r = T.rec + slot * T.stride + T.kp;
  *reinterpret_cast<RowHdr*>(r) = o;
  const int span = hdr_span(T.kp);
  for (int i = 4; i < span; i += 4) *reinterpret_cast<float4*>(r + i) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// The header an updated row leaves the step with: current through epoch + 1.  (Where a kernel
// stores it as a quad, it reinterprets the returned object in place: handing it to a further helper
// changed the register allocation of k_segment_update and the fused forward.)
__device__ __forceinline__ RowHdr next_hdr(float w_new, const StepParams& p) {
  RowHdr o;
  o.w = w_new;
  o.t = p.epoch + 1;
  o.cum = p.cum_next;
  return o;
}

// Row update of SGD.scala:150-181, fp64 soft-threshold (the combine and the replicated apply):
//   vec' = S_lambda(vec - sum * (eta / m));  strength' = S_lambda(strength - (sum / m) * eta)
__device__ __forceinline__ float upd_v(float v, double g, const StepParams& p) {
  return (float)shrink_d((double)v - g * p.scale_v, p.lam);
}
__device__ __forceinline__ float upd_w(float w, double g, const StepParams& p) {
  return (float)shrink_d((double)w - (g / p.m) * p.eta, p.lam);
}

// The same update with the fp32 soft-threshold (the fused forward's singleton rows and the
// segmented update's runs; the two must agree to the bit, so both call these).  A row's pending L1:
__device__ __forceinline__ float pending_l1(const RowHdr& h, const StepParams& p) { return (float)(p.cumE - h.cum); }
// One V quad brought current by acf and its run's gradient  g[f] = A[f] - v[f] * b  (A = sum S x r of
// the quad's columns, b = sum x^2 r), fp64.
struct QuadGrad { float4 v; double g0, g1, g2, g3; };
__device__ __forceinline__ QuadGrad quad_grad(float4 v_raw, float acf, const double* A, double b) {
  const float4 v = shrink4f(v_raw, acf);
  return QuadGrad{v, A[0] - (double)v.x * b, A[1] - (double)v.y * b, A[2] - (double)v.z * b, A[3] - (double)v.w * b};
}
// vec' = S_lambda(vec - sum * (eta / m))  (SGD.scala:153, :179)
__device__ __forceinline__ float4 quad_apply(const QuadGrad& q, const StepParams& p) {
  const float4 u = make_float4((float)fma(q.g0, -p.scale_v, (double)q.v.x), (float)fma(q.g1, -p.scale_v, (double)q.v.y),
                               (float)fma(q.g2, -p.scale_v, (double)q.v.z), (float)fma(q.g3, -p.scale_v, (double)q.v.w));
  return shrink4f(u, (float)p.lam);
}
__device__ __forceinline__ float4 upd_quad(float4 v_raw, float acf, const double* A, double b, const StepParams& p) {
  return quad_apply(quad_grad(v_raw, acf, A, b), p);
}
// strength' of the row whose header is h (SGD.scala:150, :171)
__device__ __forceinline__ float upd_w_row(const RowHdr& h, float acf, double gw, const StepParams& p) {
  return upd_w(shrink1f(h.w, acf), gw, p);
}

// Singleton rows.  fm_batch_prepare sorts the batch (side stream); at the start of the step the
// split (k_split_*, fm_update.hip, main stream) keeps the runs of two or more entries (the only ones
// that need a per-feature reduction) and marks every such row in the row header's t field, the word
// that otherwise only says present (t >= 0) or absent (t = -1):
//   present, multi at epoch E : t = kTagPresent + (E & kTagMask)   (>= 2^30; normal t < 2^30)
//   absent,  multi at epoch E : t = -2 - (E & kTagMask)            (<= -2: still "absent")
// so every reader that asks t >= 0 is unchanged, and the fused forward, which loads the header of
// every entry's row anyway, knows which rows it may update in place: nobody else reads them in
// this step.  The segmented update then walks the multi runs only and rewrites their headers
// (t = E + 1), clearing the tags.
constexpr int32_t kTagPresent = 1 << 30;
constexpr int32_t kTagMask = (1 << 29) - 1;
__device__ __forceinline__ int32_t multi_tag(int32_t epoch, bool present) {
  return present ? kTagPresent + (epoch & kTagMask) : -2 - (epoch & kTagMask);
}
__device__ __forceinline__ bool is_multi(int32_t t, int32_t epoch) {
  const int32_t e = epoch & kTagMask;
  return t >= kTagPresent ? t - kTagPresent == e : (t <= -2 && -2 - t == e);
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// N(0, sd^2) draw keyed by (seed, feature id, factor f; f = -1 for w).  Box-Muller in fp64.
__device__ __forceinline__ float gauss_draw(uint64_t seed, int64_t id, int f, double sd) {
  const uint64_t c = ((uint64_t)id << 10) ^ (uint64_t)(f + 1);
  const uint64_t h1 = splitmix64(seed ^ splitmix64(c));
  const uint64_t h2 = splitmix64(h1 ^ 0x632BE59BD9B4E019ull);
  const double u1 = (double)((h1 >> 11) + 1) * 0x1.0p-53;
  const double u2 = (double)(h2 >> 11) * 0x1.0p-53;
  const double g = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
  return (float)(g * sd);
}

}  // namespace fmhip
