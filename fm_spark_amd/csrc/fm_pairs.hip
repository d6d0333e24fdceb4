// (context, candidate) pair batches: fm_batch_from_pairs' and fm_batch_sample_pairs' device side.
//   k_pair_rows    the gather both calls share: output row s = the entries of row pair_ctx[s] of the
//                  contexts followed by those of row pair_cand[s] of the candidates
//   k_pair_sample  the sampled call's pairs: each positive, then its n_neg drawn candidate rows, with
//                  every output row's label and length
//   k_pair_sample_hard  fm_batch_sample_pairs_hard's pairs: n_draw draws per positive scored against a
//                  summary snapshot, the best n_neg kept (a wave per positive; its comment below).  The draw
//                  is its parameter: the uniform one, or fm_batch_sample_pairs_weighted's (fm_weights.hip)
//   k_pair_chunk_sum / k_pair_scan_chunks / k_pair_scan_rows
//                  the exclusive scan of those lengths into the result's row_ptr, in the three phases
//                  of fm_update.hip's split: chunk totals, a one-block scan of the totals (in rounds),
//                  each chunk's local scan plus its offset (launch_len_scan: also the scan of
//                  fm_lists_from_pairs' head flags, fm_lists.hip)
// Integer work and copies only, no atomics: equal inputs give equal bits.
//
// The sampled call's scratch (PairWork, fm_internal.h: the lists' device copies, the drawn pairs, the
// labels, lengths, row_ptr and the scan's chunk arrays) belongs to the context and is touched on the
// context's copy stream alone: the uploads, these kernels, the read-back of the total and the gather
// that reads the pairs are all enqueued there, so a call's writes queue behind the previous call's
// gather (copy-stream order) and no event or host wait protects the scratch between calls.  The one
// exception is the score-aware call's summary snapshot (PairWork::snap_*): written on the main stream by a
// refreshing call, read on the copy stream, and ordered by the two events fm_capi.hip records around it.
#include <algorithm>

#include "fm_device.h"

namespace fmhip {

// One team of 16 lanes per output row, as k_select_rows: the row's first len_u entries are the context
// row's ids and fp32 x, the rest the candidate row's (both contiguous, 8 B per entry), written with the
// exploded {s, x} entries; row_ptr (rp_in: computed by the host, or by the scan below) and the labels
// are copied alongside (grid-stride, the same pass).
__global__ __launch_bounds__(kBlock) void k_pair_rows(const int32_t* __restrict__ pair_ctx, const int32_t* __restrict__ pair_cand,
                                                     const int64_t* __restrict__ rp_in, const double* __restrict__ lab_in,
                                                     const int64_t* __restrict__ u_rp, const uint32_t* __restrict__ u_col,
                                                     const float* __restrict__ u_xs, const int64_t* __restrict__ c_rp,
                                                     const uint32_t* __restrict__ c_col, const float* __restrict__ c_xs,
                                                     int64_t B, int64_t* __restrict__ rp, double* __restrict__ lab,
                                                     uint32_t* __restrict__ col, uint2* __restrict__ ent,
                                                     float* __restrict__ xs) {
  constexpr int T = 16;
  const int tl = threadIdx.x % T;
  const int64_t gtid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = gtid; i <= B; i += nthreads) rp[i] = rp_in[i];
  for (int64_t i = gtid; i < B; i += nthreads) lab[i] = lab_in[i];
  for (int64_t s = gtid / T; s < B; s += nthreads / T) {
    const int64_t e0 = rp_in[s], e1 = rp_in[s + 1];
    const int64_t u = pair_ctx[s], c = pair_cand[s];
    const int64_t su = u_rp[u], lu = u_rp[u + 1] - su;
    const int64_t sc = c_rp[c], lc = c_rp[c + 1] - sc;
    for (int64_t j = tl; j < e1 - e0; j += T) {
      uint32_t id;
      float x;
      if (j < lu) {
        id = u_col[su + j];
        x = u_xs[su + j];
      } else if (j - lu < lc) {
        id = c_col[sc + j - lu];
        x = c_xs[sc + j - lu];
      } else {
        break;  // (rp_in is the scan of lu + lc: not reached)
      }
      col[e0 + j] = id;
      xs[e0 + j] = x;
      ent[e0 + j] = make_uint2((uint32_t)s, __float_as_uint(x));
    }
  }
}

// One thread per output row r = i (1 + n_neg) + jj of the sampled call: jj = 0 is positive i's own pair
// with pos_label; jj = 1 + j its j-th negative with neg_label, the candidate row
//   h = splitmix64(seed ^ splitmix64((i << 20) | j));  r = ((h >> 32) * E) >> 32;  c = r + #{t : excl[t] - t <= r}
// -- the r-th row, ascending, of [0, C) without the context's strictly ascending exclude list (E = C -
// its length; excl[t] - t does not decrease, so the count is a binary search).  A function of (seed, i,
// j), the list and C alone.  len[r] = the two rows' entries together.
__global__ __launch_bounds__(kBlock) void k_pair_sample(const int32_t* __restrict__ pos_ctx, const int32_t* __restrict__ pos_cand,
                                                       int64_t B, int32_t n_neg, const int64_t* __restrict__ excl_ptr,
                                                       const int32_t* __restrict__ excl_rows, int64_t C, double pos_label,
                                                       double neg_label, uint64_t seed, const int64_t* __restrict__ u_rp,
                                                       const int64_t* __restrict__ c_rp, int32_t* __restrict__ pair_ctx,
                                                       int32_t* __restrict__ pair_cand, double* __restrict__ lab,
                                                       uint32_t* __restrict__ len) {
  const int64_t per = (int64_t)n_neg + 1;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < B; r += (int64_t)gridDim.x * kBlock) {
    const int64_t i = r / per, jj = r - i * per;
    const int64_t u = pos_ctx[i];
    int64_t c;
    if (jj == 0) {
      c = pos_cand[i];
    } else {
      const int64_t x0 = excl_ptr ? excl_ptr[u] : 0, L = excl_ptr ? excl_ptr[u + 1] - x0 : 0;
      const uint64_t E = (uint64_t)(C - L);
      const uint64_t h = splitmix64(seed ^ splitmix64(((uint64_t)i << 20) | (uint64_t)(jj - 1)));
      const int64_t d = (int64_t)(((h >> 32) * E) >> 32);
      int64_t lo = 0, hi = L;  // the first t with excl[t] - t > d
      while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        if ((int64_t)excl_rows[x0 + mid] - mid <= d) lo = mid + 1;
        else hi = mid;
      }
      c = d + lo;
    }
    pair_ctx[r] = (int32_t)u;
    pair_cand[r] = (int32_t)c;
    lab[r] = jj == 0 ? pos_label : neg_label;
    len[r] = (uint32_t)((u_rp[u + 1] - u_rp[u]) + (c_rp[c + 1] - c_rp[c]));
  }
}

// ---- fm_batch_sample_pairs_hard: score-aware negatives.  Per positive i the n_draw candidate rows c_ij of
// k_pair_sample's contract are scored against the context by score_row (fm_device.h: the ranking calls'
// 64-bit keys, from the summary snapshot the call hands in) and the n_neg that come first under (larger key,
// then smaller j) are emitted in ascending j.  The order is total, so the result is a function of (seed, i,
// the list, C, the snapshot) alone; with n_neg == n_draw every draw is kept and the output is k_pair_sample's.
//
// One wave per positive, grid-stride, kHardWaves or kHardWavesWide waves per block; a wave owns a slice of
// the block's dynamic LDS and never meets another wave, so there is no block barrier, only wave_lds_sync.
//   stage   S_u (kp doubles) into the slice; w0 + a_u and "u has a learned entry" into registers
//   draw    lane l takes the draws j = l, l + 64, ...: the hash, the binary search over the exclude list, then
//           the kp-long fp64 fma chain over the candidate's summary row (score_row)
//   select  n_draw <= 64: a draw per lane, all in registers.  Each lane counts the draws that come before
//           its own -- n_draw broadcasts of a (key, j) pair -- and is kept when that rank is below n_neg: the
//           flags come out in j order, so nothing is permuted and nothing goes through LDS.  (A register
//           bitonic sort takes 21 exchange stages of three shuffles each whatever n_draw is, and its result
//           has to be un-permuted back into j order; the count takes n_draw broadcasts, 16 at the usual size.)
//           n_draw > 64: (key, j) pairs into the slice, padded to the next power of two P with (kWorstKey,
//           0xFFFFFFFF), a wave-level bitonic sort (descending), then the first n_neg entries flag bit 31 of
//           their draw's slot in the slice's candidate array (indexed by j, never permuted; c < 2^31)
//   emit    in rounds of 64 draws in j order: ballot of the flags, popcount of the lanes below = the slot
//           among the positive's negatives; pair_ctx, pair_cand, lab, len of row i (1 + n_neg) + 1 + slot.
//           Lane 0 writes the positive's own row.
// LDS per wave: 8 kp bytes, and 16 P bytes beyond 64 draws; P <= 512 runs four waves per block (40 KiB at
// most), P = 1024 two (36 KiB), so no launch needs more than the default 64 KiB of dynamic LDS.
// Integers and fp64 only, no atomics, one writer per slot.
constexpr int kHardMaxDraw = 1024;   // n_draw, at most
constexpr int kHardWaves = 4;        // waves per block ...
constexpr int kHardWavesWide = 2;    // ... and once a slice holds more than 512 draws
static_assert(kHardWaves * 64 <= kBlock && kHardMaxDraw % 64 == 0, "whole rounds of 64 draws; a block of at most kBlock");

// draw j of positive i (k_pair_sample's arithmetic): the d-th row, ascending, of [0, C) without the list
// excl_rows[x0, x0 + L)
__device__ __forceinline__ int64_t pair_draw(uint64_t seed, int64_t i, int64_t j, const int32_t* __restrict__ excl_rows,
                                             int64_t x0, int64_t L, int64_t C) {
  const uint64_t E = (uint64_t)(C - L);
  const uint64_t h = splitmix64(seed ^ splitmix64(((uint64_t)i << 20) | (uint64_t)j));
  const int64_t d = (int64_t)(((h >> 32) * E) >> 32);
  int64_t lo = 0, hi = L;  // the first t with excl[t] - t > d
  while (lo < hi) {
    const int64_t mid = (lo + hi) / 2;
    if ((int64_t)excl_rows[x0 + mid] - mid <= d) lo = mid + 1;
    else hi = mid;
  }
  return d + lo;
}

// The draw as k_pair_sample_hard's parameter: draw j of positive i with context u, whose list is entries
// [x0, x0 + L) of the call's lists.  UniformPairDraw is pair_draw; WeightedPairDraw the weighted contract's
// (fm_device.h: two binary searches, the second over the whole cdf -- a wave per positive has no block-wide
// pivot table, and its draws are a small part of a selection that scores every one of them).
struct UniformPairDraw {
  const int32_t* excl_rows;
  int64_t C;
  __device__ __forceinline__ int64_t operator()(uint64_t seed, int64_t i, int64_t j, int64_t u, int64_t x0, int64_t L) const {
    return pair_draw(seed, i, j, excl_rows, x0, L, C);
  }
};
struct WeightedPairDraw {
  WeightedDraw d;
  int64_t C;
  __device__ __forceinline__ int64_t operator()(uint64_t seed, int64_t i, int64_t j, int64_t u, int64_t x0, int64_t L) const {
    const uint64_t v = weighted_target(seed, i, j, d.kx, x0, L, d.ew ? (uint64_t)d.ew[u] : d.W);
    return weighted_row(d.cdf, v, 1, C);
  }
};

// the summary snapshot and the two sources' row offsets, as the kernel reads them
struct HardSources {
  const double* sum_u;
  const double* bias_u;
  const uint32_t* cnt_u;
  const double* sum_c;
  const double* bias_c;
  const uint32_t* cnt_c;
  const int64_t* u_rp;
  const int64_t* c_rp;
};

// kWide: n_draw > 64 (a kernel each: together they spill SGPRs); Draw: UniformPairDraw or WeightedPairDraw
template <int kWaves, bool kWide, class Draw>
__global__ __launch_bounds__(kWaves * 64) void k_pair_sample_hard(
    const int32_t* __restrict__ pos_ctx, const int32_t* __restrict__ pos_cand, int64_t n_pos, int32_t n_neg, int32_t n_draw,
    int32_t P, const int64_t* __restrict__ excl_ptr, Draw draw, double pos_label,
    double neg_label, uint64_t seed, HardSources s, int kp, double w0, int32_t* __restrict__ pair_ctx,
    int32_t* __restrict__ pair_cand, double* __restrict__ lab, uint32_t* __restrict__ len) {
  extern __shared__ __align__(16) unsigned char hard_lds[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr bool wide = kWide;
  const size_t slice = sizeof(double) * (size_t)kp + (wide ? (size_t)16 * P : 0);
  double* su = reinterpret_cast<double*>(hard_lds + slice * wave);
  uint64_t* key = reinterpret_cast<uint64_t*>(su + kp);                 // [P]
  uint32_t* idx = reinterpret_cast<uint32_t*>(key + (wide ? P : 0));    // [P]: the draw j of a sorted entry
  uint32_t* cand = idx + (wide ? P : 0);                                // [P]: c of draw j; bit 31 = kept
  const uint64_t below = (1ull << lane) - 1;
  const int64_t per = (int64_t)n_neg + 1;
  for (int64_t i = (int64_t)blockIdx.x * kWaves + wave; i < n_pos; i += (int64_t)gridDim.x * kWaves) {
    wave_lds_sync();  // the slice's previous positive has been read
    const int64_t u = pos_ctx[i];
    for (int f = lane; f < kp; f += 64) su[f] = s.sum_u[u * kp + f];
    const RankContext x = {w0 + s.bias_u[u], s.cnt_u[u] != 0, 0, 0};
    const int64_t x0 = excl_ptr ? excl_ptr[u] : 0, L = excl_ptr ? excl_ptr[u + 1] - x0 : 0;
    const int64_t lu = s.u_rp[u + 1] - s.u_rp[u];
    const int64_t r0 = i * per;
    if (lane == 0) {
      const int64_t c = pos_cand[i];
      pair_ctx[r0] = (int32_t)u;
      pair_cand[r0] = (int32_t)c;
      lab[r0] = pos_label;
      len[r0] = (uint32_t)(lu + (s.c_rp[c + 1] - s.c_rp[c]));
    }
    wave_lds_sync();  // S_u is staged
    // one round of the emit: this lane's draw (row c, kept or not) -> its slot behind the `done` kept before
    auto emit = [&](bool kept, int64_t c, int done) {
      const uint64_t m = __ballot(kept);
      if (kept) {
        const int64_t r = r0 + 1 + done + __popcll(m & below);
        pair_ctx[r] = (int32_t)u;
        pair_cand[r] = (int32_t)c;
        lab[r] = neg_label;
        len[r] = (uint32_t)(lu + (s.c_rp[c + 1] - s.c_rp[c]));
      }
      return done + (int)__popcll(m);
    };
    if constexpr (!wide) {
      uint64_t k = kWorstKey;
      int64_t c = 0;
      if (lane < n_draw) {
        c = draw(seed, i, lane, u, x0, L);
        k = score_row(su, x, s.sum_c, s.bias_c, s.cnt_c, c, kp, w0);
      }
      int rank = 0;  // the draws that come before this lane's
      for (int j = 0; j < n_draw; ++j) rank += before(__shfl(k, j), (uint32_t)j, k, (uint32_t)lane) ? 1 : 0;
      emit(lane < n_draw && rank < n_neg, c, 0);
      continue;
    }
    for (int j = lane; j < P; j += 64) {
      uint64_t k = kWorstKey;
      uint32_t c = 0;
      if (j < n_draw) {
        c = (uint32_t)draw(seed, i, j, u, x0, L);
        k = score_row(su, x, s.sum_c, s.bias_c, s.cnt_c, c, kp, w0);
      }
      key[j] = k;
      idx[j] = j < n_draw ? (uint32_t)j : 0xFFFFFFFFu;
      cand[j] = c;
    }
    wave_lds_sync();
    // bitonic sort of (key, idx), descending: partner distance d inside blocks of kk (fm_rank.hip's bitonic_stage,
    // a wave's worth)
    for (int kk = 2; kk <= P; kk <<= 1) {
      for (int d = kk >> 1; d > 0; d >>= 1) {
        for (int t = lane; t < P / 2; t += 64) {
          const int a = ((t & ~(d - 1)) << 1) | (t & (d - 1));
          const int b = a | d;
          const uint64_t ka = key[a], kb = key[b];
          const uint32_t ia = idx[a], ib = idx[b];
          const bool desc = (a & kk) == 0;
          if (before(kb, ib, ka, ia) == desc) {
            key[a] = kb; idx[a] = ib;
            key[b] = ka; idx[b] = ia;
          }
        }
        wave_lds_sync();
      }
    }
    for (int t = lane; t < n_neg; t += 64) cand[idx[t]] |= 0x80000000u;  // distinct j: one writer per slot
    wave_lds_sync();
    int done = 0;
    for (int j0 = 0; j0 < n_draw; j0 += 64) {
      const int j = j0 + lane;
      const uint32_t cj = j < n_draw ? cand[j] : 0;
      done = emit((cj >> 31) != 0, (int64_t)(cj & 0x7FFFFFFFu), done);
    }
  }
}

// The scan of the lengths.  A chunk is one block's worth of rows, a thread per row; the chunk totals
// are scanned by one block, kPairScanNT threads with kPairScanPer consecutive totals each per round.
constexpr int kPairChunk = kBlock;    // rows per scan chunk
constexpr int kPairScanNT = 256;      // threads of the one-block scan of the chunk totals
constexpr int kPairScanPer = 4;       // chunk totals per thread and round
static_assert(kPairChunk == 256, "the scan's chunk edges tests/test_gpu_pairs.py and tests/test_gpu_row_lists.py place their counts at");
static_assert(kPairChunk == kBlock, "k_pair_chunk_sum / k_pair_scan_rows give every row of a chunk one thread of a block");
static_assert(kPairChunk % 64 == 0 && kPairScanNT % 64 == 0, "whole waves: the block scans combine per-wave sums");
static_assert(kPairScanNT <= 1024 && kPairScanPer >= 1, "one block scans a round");
// a round takes kPairScanNT * kPairScanPer = 1024 chunks = 262 144 rows: the step's batch in one round
static_assert((int64_t)kPairScanNT * kPairScanPer * kPairChunk == 262144, "rows per round of the chunk-total scan (tests/test_gpu_pairs.py)");

// (block_scan_incl: fm_device.h, shared with fm_weights.hip's tile scan)

// phase 1: tot[c] = the lengths of chunk c summed
__global__ __launch_bounds__(kBlock) void k_pair_chunk_sum(const uint32_t* __restrict__ len, int64_t B, int64_t nchunks,
                                                          int64_t* __restrict__ tot) {
  __shared__ int64_t ws[kBlock / 64];
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {  // block-uniform
    const int64_t i = c * kPairChunk + threadIdx.x;
    int64_t t = 0;
    block_scan_incl<kBlock / 64>(i < B ? (int64_t)len[i] : 0, ws, &t);
    if (threadIdx.x == 0) tot[c] = t;
  }
}

// phase 2, one block: off[c] = the totals before chunk c; the grand total -> rp[B] (the result's last
// row_ptr slot) and total[0] (read back by the host)
__global__ __launch_bounds__(kPairScanNT) void k_pair_scan_chunks(const int64_t* __restrict__ tot, int64_t nchunks,
                                                                 int64_t* __restrict__ off, int64_t* __restrict__ rp_last,
                                                                 int64_t* __restrict__ total) {
  __shared__ int64_t ws[kPairScanNT / 64];
  int64_t carry = 0;
  for (int64_t b = 0; b < nchunks; b += (int64_t)kPairScanNT * kPairScanPer) {
    const int64_t i0 = b + (int64_t)threadIdx.x * kPairScanPer;
    int64_t v[kPairScanPer];
#pragma unroll
    for (int j = 0; j < kPairScanPer; ++j) v[j] = i0 + j < nchunks ? tot[i0 + j] : 0;
    int64_t t = 0;
#pragma unroll
    for (int j = 0; j < kPairScanPer; ++j) t += v[j];
    int64_t round = 0;
    int64_t run = carry + block_scan_incl<kPairScanNT / 64>(t, ws, &round) - t;
#pragma unroll
    for (int j = 0; j < kPairScanPer; ++j) {
      if (i0 + j < nchunks) off[i0 + j] = run;
      run += v[j];
    }
    carry += round;
  }
  if (threadIdx.x == 0) {
    *rp_last = carry;
    *total = carry;
  }
}

// phase 3: rp[i] = off[chunk of i] + the lengths before i in its chunk
__global__ __launch_bounds__(kBlock) void k_pair_scan_rows(const uint32_t* __restrict__ len, int64_t B, int64_t nchunks,
                                                          const int64_t* __restrict__ off, int64_t* __restrict__ rp) {
  __shared__ int64_t ws[kBlock / 64];
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {  // block-uniform
    const int64_t i = c * kPairChunk + threadIdx.x;
    const int64_t l = i < B ? (int64_t)len[i] : 0;
    int64_t t = 0;
    const int64_t incl = block_scan_incl<kBlock / 64>(l, ws, &t);
    if (i < B) rp[i] = off[c] + incl - l;
  }
}

void launch_pair_rows(const int32_t* pair_ctx, const int32_t* pair_cand, const int64_t* row_ptr_in, const double* label_in,
                      const BatchDev& contexts, const BatchDev& candidates, int64_t B, BatchDev& dst, hipStream_t st) {
  hipLaunchKernelGGL(k_pair_rows, dim3(grid_for(std::max<int64_t>(B, 1) * 16, kBlock, 256 * 8)), dim3(kBlock), 0, st, pair_ctx,
                     pair_cand, row_ptr_in, label_in, contexts.row_ptr.as<int64_t>(), contexts.col.as<uint32_t>(),
                     contexts.xs.as<float>(), candidates.row_ptr.as<int64_t>(), candidates.col.as<uint32_t>(),
                     candidates.xs.as<float>(), B, dst.row_ptr.as<int64_t>(), dst.label.as<double>(), dst.col.as<uint32_t>(),
                     dst.ent.as<uint2>(), dst.xs.as<float>());
  FM_HIP_CHECK(hipGetLastError());
}

int64_t pair_scan_chunks(int64_t B) { return (B + kPairChunk - 1) / kPairChunk; }

void launch_pair_sample(const int32_t* pos_ctx, const int32_t* pos_cand, int64_t n_pos, int32_t n_neg, const int64_t* excl_ptr,
                        const int32_t* excl_rows, double pos_label, double neg_label, uint64_t seed, const BatchDev& contexts,
                        const BatchDev& candidates, int32_t* pair_ctx, int32_t* pair_cand, double* label, uint32_t* len,
                        int64_t* row_ptr, int64_t* chunk_tot, int64_t* chunk_off, int64_t* total, hipStream_t st) {
  const int64_t B = n_pos * ((int64_t)n_neg + 1);
  if (B <= 0) {
    FM_HIP_CHECK(hipMemsetAsync(row_ptr, 0, sizeof(int64_t), st));
    FM_HIP_CHECK(hipMemsetAsync(total, 0, sizeof(int64_t), st));
    return;
  }
  hipLaunchKernelGGL(k_pair_sample, dim3(grid_for(B, kBlock)), dim3(kBlock), 0, st, pos_ctx, pos_cand, B, n_neg, excl_ptr,
                     excl_rows, candidates.n_rows, pos_label, neg_label, seed, contexts.row_ptr.as<int64_t>(),
                     candidates.row_ptr.as<int64_t>(), pair_ctx, pair_cand, label, len);
  launch_len_scan(len, B, row_ptr, chunk_tot, chunk_off, total, st);
}

// both draws' launch: the kernel by n_draw, then the lengths' scan
template <class Draw>
static void launch_hard(const Draw& draw, const int32_t* pos_ctx, const int32_t* pos_cand, int64_t n_pos, int32_t n_neg,
                        int32_t n_draw, const int64_t* excl_ptr, double pos_label, double neg_label, uint64_t seed,
                        const BatchDev& contexts, const BatchDev& candidates, const RankSide& su, const RankSide& sc, int kp,
                        double w0, int32_t* pair_ctx, int32_t* pair_cand, double* label, uint32_t* len, int64_t* row_ptr,
                        int64_t* chunk_tot, int64_t* chunk_off, int64_t* total, hipStream_t st) {
  const int64_t B = n_pos * ((int64_t)n_neg + 1);
  if (B <= 0) {
    launch_len_scan(len, 0, row_ptr, chunk_tot, chunk_off, total, st);
    return;
  }
  int P = 64;  // the slice's sorted entries: the power of two that holds n_draw (not read up to 64 draws)
  while (P < n_draw) P <<= 1;
  const HardSources s = {su.sum, su.bias, su.cnt, sc.sum, sc.bias, sc.cnt, contexts.row_ptr.as<int64_t>(),
                         candidates.row_ptr.as<int64_t>()};
  const size_t slice = sizeof(double) * (size_t)kp + (n_draw > 64 ? (size_t)16 * P : 0);
  const auto launch = [&](auto kern, int waves) {
    const int64_t blocks = (n_pos + waves - 1) / waves;
    hipLaunchKernelGGL(kern, dim3(grid_for(blocks * waves * 64, waves * 64, 256 * 8)), dim3(waves * 64), slice * waves, st,
                       pos_ctx, pos_cand, n_pos, n_neg, n_draw, P, excl_ptr, draw, pos_label, neg_label,
                       seed, s, kp, w0, pair_ctx, pair_cand, label, len);
  };
  if (n_draw <= 64) launch(k_pair_sample_hard<kHardWaves, false, Draw>, kHardWaves);
  else if (P <= 512) launch(k_pair_sample_hard<kHardWaves, true, Draw>, kHardWaves);
  else launch(k_pair_sample_hard<kHardWavesWide, true, Draw>, kHardWavesWide);
  launch_len_scan(len, B, row_ptr, chunk_tot, chunk_off, total, st);
}

void launch_pair_sample_hard(const int32_t* pos_ctx, const int32_t* pos_cand, int64_t n_pos, int32_t n_neg, int32_t n_draw,
                             const int64_t* excl_ptr, const int32_t* excl_rows, double pos_label, double neg_label,
                             uint64_t seed, const BatchDev& contexts, const BatchDev& candidates, const RankSide& su,
                             const RankSide& sc, int kp, double w0, int32_t* pair_ctx, int32_t* pair_cand, double* label,
                             uint32_t* len, int64_t* row_ptr, int64_t* chunk_tot, int64_t* chunk_off, int64_t* total,
                             hipStream_t st) {
  launch_hard(UniformPairDraw{excl_rows, candidates.n_rows}, pos_ctx, pos_cand, n_pos, n_neg, n_draw, excl_ptr, pos_label,
              neg_label, seed, contexts, candidates, su, sc, kp, w0, pair_ctx, pair_cand, label, len, row_ptr, chunk_tot,
              chunk_off, total, st);
}

void launch_pair_sample_hard_weighted(const int32_t* pos_ctx, const int32_t* pos_cand, int64_t n_pos, int32_t n_neg,
                                      int32_t n_draw, const int64_t* excl_ptr, const WeightedDraw& d, double pos_label,
                                      double neg_label, uint64_t seed, const BatchDev& contexts, const BatchDev& candidates,
                                      const RankSide& su, const RankSide& sc, int kp, double w0, int32_t* pair_ctx,
                                      int32_t* pair_cand, double* label, uint32_t* len, int64_t* row_ptr,
                                      int64_t* chunk_tot, int64_t* chunk_off, int64_t* total, hipStream_t st) {
  launch_hard(WeightedPairDraw{d, candidates.n_rows}, pos_ctx, pos_cand, n_pos, n_neg, n_draw, excl_ptr, pos_label,
              neg_label, seed, contexts, candidates, su, sc, kp, w0, pair_ctx, pair_cand, label, len, row_ptr, chunk_tot,
              chunk_off, total, st);
}

void launch_len_scan(const uint32_t* len, int64_t B, int64_t* off, int64_t* chunk_tot, int64_t* chunk_off, int64_t* total,
                     hipStream_t st) {
  if (B <= 0) {
    FM_HIP_CHECK(hipMemsetAsync(off, 0, sizeof(int64_t), st));
    FM_HIP_CHECK(hipMemsetAsync(total, 0, sizeof(int64_t), st));
    return;
  }
  const int64_t nchunks = pair_scan_chunks(B);
  const unsigned blocks = grid_for(nchunks * kBlock, kBlock);
  hipLaunchKernelGGL(k_pair_chunk_sum, dim3(blocks), dim3(kBlock), 0, st, len, B, nchunks, chunk_tot);
  hipLaunchKernelGGL(k_pair_scan_chunks, dim3(1), dim3(kPairScanNT), 0, st, chunk_tot, nchunks, chunk_off, off + B, total);
  hipLaunchKernelGGL(k_pair_scan_rows, dim3(blocks), dim3(kBlock), 0, st, len, B, nchunks, chunk_off, off);
  FM_HIP_CHECK(hipGetLastError());
}


}  // namespace fmhip
