// Popularity-weighted negatives: fm_row_weights_bind's and fm_batch_sample_pairs_weighted's device side.
// (The weights' cdf is launch_len_scan of the weights themselves, fm_pairs.hip: no kernel of its own.)
//   k_weights_bind_short / k_weights_bind_long
//                  the binding of a weights object to one set of exclude lists: per context the exclusive
//                  scan X_t of weight[e_t] over its list e_0 < e_1 < ..., kept per list entry as
//                  kx[t] = {key_t = cdf[e_t] - X_t, X_{t + 1}}, and the context's eligible weight
//                  ew[u] = W - X_L.  key_t is the eligible weight below row e_t: it does not decrease in t,
//                  and it is what the draw searches.
//   k_pair_sample_weighted
//                  k_pair_sample with the weighted draw: r in [0, E_w), t* = #{t : key_t <= r}, then the row
//                  c with cdf[c] <= r + X_{t*} < cdf[c + 1].
// Integer work only, every slot with exactly one writer, no atomics: equal inputs give equal bytes.
//
// The scan's geometry.  The lists of one call run from empty to every candidate row, and nearly all are short:
//   L <= kBindShort (64)   a team of kBindTeam = 16 lanes per list, four lists to a wave, in
//                          kBindShort / kBindTeam = 4 rounds of a 16-wide __shfl_up scan with the running sum
//                          carried from round to round.  The rounds are unconditional (loads predicated), so a
//                          wave's four teams never diverge around a shuffle.  A whole wave per list would idle
//                          three lanes in four at the usual lengths (a few dozen rows).
//   L >  kBindShort        a block per list (the host lists those contexts from its copy of the offsets: their
//                          number sizes the grid), walking the list in tiles of kBindTile = 1024 rows, four
//                          consecutive rows per thread; a tile is the threads' sums scanned over the block
//                          (block_scan_incl) plus the carry of the tiles before it.
// All sums are below 2^32 (a list's rows are distinct, so X_t <= W), held in 64 bits and stored in 32.
//
// The draw's two dependent searches.  A thread per output row, as k_pair_sample: the 1 + n_neg rows of a
// positive are neighbours in a wave and share the context, so their probes of its kx entries fall into the
// same lines (the first probes are the same address: one request).  The cdf search's top levels would be the
// same ten probes for every thread of the grid: each block stages kPivots = 1024 pivots cdf[k stride],
// stride = ceil(C / 1024), once into 4 KiB of LDS (as uint32: cdf < 2^32), searches them there, and only the
// last ~log2(stride) probes go to memory, inside one stride of the cdf.  Up to 1024 candidate rows the cdf is
// the pivot table and the search never leaves LDS.
#include <algorithm>

#include "fm_device.h"

namespace fmhip {

constexpr int kBindTeam = 16;                     // lanes per short list
constexpr int kBindPer = kBindTile / kBlock;      // rows per thread and tile of a long list
constexpr int kPivots = 1024;                     // pivots of the cdf search in LDS, at most
static_assert(kBindShort % kBindTeam == 0 && 64 % kBindTeam == 0, "whole rounds; whole teams per wave");
static_assert(kBindTile == kBlock * kBindPer && kBindPer >= 1, "a tile is kBindPer rows of every thread of a block");

__global__ __launch_bounds__(kBlock) void k_weights_bind_short(const uint32_t* __restrict__ weight, const int64_t* __restrict__ cdf,
                                                              uint64_t W, const int64_t* __restrict__ excl_ptr,
                                                              const int32_t* __restrict__ excl_rows, int64_t U,
                                                              uint2* __restrict__ kx, uint32_t* __restrict__ ew) {
  constexpr int T = kBindTeam, per_wave = 64 / T;
  const int lane = threadIdx.x & 63, tl = lane % T;
  const int64_t wave = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * kBlock) >> 6;
  for (int64_t ub = wave * per_wave; ub < U; ub += nwaves * per_wave) {  // wave-uniform
    const int64_t u = ub + lane / T;
    const bool live = u < U;
    const int64_t x0 = live ? excl_ptr[u] : 0, L = live ? excl_ptr[u + 1] - x0 : 0;
    const bool mine = live && L <= kBindShort;
    uint64_t carry = 0;  // X at the round's first entry
#pragma unroll
    for (int t0 = 0; t0 < kBindShort; t0 += T) {
      const int t = t0 + tl;
      const bool on = mine && t < L;
      const int64_t e = on ? excl_rows[x0 + t] : 0;
      const uint64_t w = on ? weight[e] : 0;
      uint64_t v = w;
#pragma unroll
      for (int o = 1; o < T; o <<= 1) {
        const uint64_t below = __shfl_up(v, o, T);
        if (tl >= o) v += below;
      }
      if (on) kx[x0 + t] = make_uint2((uint32_t)((uint64_t)cdf[e] - (carry + v - w)), (uint32_t)(carry + v));
      carry += __shfl(v, T - 1, T);
    }
    if (mine && tl == 0) ew[u] = (uint32_t)(W - carry);
  }
}

__global__ __launch_bounds__(kBlock) void k_weights_bind_long(const uint32_t* __restrict__ weight, const int64_t* __restrict__ cdf,
                                                             uint64_t W, const int64_t* __restrict__ excl_ptr,
                                                             const int32_t* __restrict__ excl_rows,
                                                             const int32_t* __restrict__ long_ctx, int64_t n_long,
                                                             uint2* __restrict__ kx, uint32_t* __restrict__ ew) {
  __shared__ int64_t ws[kBlock / 64];
  for (int64_t k = blockIdx.x; k < n_long; k += gridDim.x) {  // block-uniform
    const int64_t u = long_ctx[k];
    const int64_t x0 = excl_ptr[u], L = excl_ptr[u + 1] - x0;
    int64_t carry = 0;  // X at the tile's first entry
    for (int64_t t0 = 0; t0 < L; t0 += kBindTile) {  // block-uniform
      const int64_t tb = t0 + (int64_t)threadIdx.x * kBindPer;
      int64_t e[kBindPer], w[kBindPer], s = 0;
#pragma unroll
      for (int q = 0; q < kBindPer; ++q) {
        const bool on = tb + q < L;
        e[q] = on ? excl_rows[x0 + tb + q] : 0;
        w[q] = on ? (int64_t)weight[e[q]] : 0;
        s += w[q];
      }
      int64_t tile = 0;
      int64_t run = carry + block_scan_incl<kBlock / 64>(s, ws, &tile) - s;
#pragma unroll
      for (int q = 0; q < kBindPer; ++q) {
        if (tb + q < L) kx[x0 + tb + q] = make_uint2((uint32_t)(cdf[e[q]] - run), (uint32_t)(run + w[q]));
        run += w[q];
      }
      carry += tile;
    }
    if (threadIdx.x == 0) ew[u] = (uint32_t)(W - (uint64_t)carry);
  }
}

// stride: rows between two pivots; np = ceil(C / stride) <= kPivots pivots piv[k] = cdf[k stride]
__global__ __launch_bounds__(kBlock) void k_pair_sample_weighted(const int32_t* __restrict__ pos_ctx, const int32_t* __restrict__ pos_cand,
                                                                int64_t B, int32_t n_neg, const int64_t* __restrict__ excl_ptr,
                                                                WeightedDraw d, int64_t C, int64_t stride, int np,
                                                                double pos_label, double neg_label, uint64_t seed,
                                                                const int64_t* __restrict__ u_rp, const int64_t* __restrict__ c_rp,
                                                                int32_t* __restrict__ pair_ctx, int32_t* __restrict__ pair_cand,
                                                                double* __restrict__ lab, uint32_t* __restrict__ len) {
  __shared__ uint32_t piv[kPivots];
  if (n_neg > 0)
    for (int k = threadIdx.x; k < np; k += kBlock) piv[k] = (uint32_t)d.cdf[(int64_t)k * stride];
  __syncthreads();
  const int64_t per = (int64_t)n_neg + 1;
  for (int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x; r < B; r += (int64_t)gridDim.x * kBlock) {
    const int64_t i = r / per, jj = r - i * per;
    const int64_t u = pos_ctx[i];
    int64_t c;
    if (jj == 0) {
      c = pos_cand[i];
    } else {
      const int64_t x0 = excl_ptr ? excl_ptr[u] : 0, L = excl_ptr ? excl_ptr[u + 1] - x0 : 0;
      const uint64_t v = weighted_target(seed, i, jj - 1, d.kx, x0, L, d.ew ? (uint64_t)d.ew[u] : d.W);
      int lo = 0, hi = np;  // the first pivot above v (piv[0] = 0 <= v: at least 1)
      while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if ((uint64_t)piv[mid] <= v) lo = mid + 1;
        else hi = mid;
      }
      // cdf[(lo - 1) stride] <= v < cdf[lo stride] (or cdf[C] = W behind the last pivot)
      const int64_t a = (int64_t)(lo - 1) * stride;
      c = weighted_row(d.cdf, v, a + 1, std::min<int64_t>(a + stride, C));
    }
    pair_ctx[r] = (int32_t)u;
    pair_cand[r] = (int32_t)c;
    lab[r] = jj == 0 ? pos_label : neg_label;
    len[r] = (uint32_t)((u_rp[u + 1] - u_rp[u]) + (c_rp[c + 1] - c_rp[c]));
  }
}

void launch_weights_bind(const uint32_t* weight, const int64_t* cdf, uint64_t W, const int64_t* excl_ptr,
                         const int32_t* excl_rows, int64_t U, const int32_t* long_ctx, int64_t n_long, uint2* kx,
                         uint32_t* ew, hipStream_t st) {
  if (U <= 0) return;
  constexpr int per_block = kBlock / kBindTeam;
  hipLaunchKernelGGL(k_weights_bind_short, dim3(grid_for((U + per_block - 1) / per_block * kBlock, kBlock)), dim3(kBlock), 0, st,
                     weight, cdf, W, excl_ptr, excl_rows, U, kx, ew);
  if (n_long > 0)
    hipLaunchKernelGGL(k_weights_bind_long, dim3(grid_for(n_long * kBlock, kBlock)), dim3(kBlock), 0, st, weight, cdf, W,
                       excl_ptr, excl_rows, long_ctx, n_long, kx, ew);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_pair_sample_weighted(const int32_t* pos_ctx, const int32_t* pos_cand, int64_t n_pos, int32_t n_neg,
                                 const int64_t* excl_ptr, const WeightedDraw& d, double pos_label, double neg_label,
                                 uint64_t seed, const BatchDev& contexts, const BatchDev& candidates, int32_t* pair_ctx,
                                 int32_t* pair_cand, double* label, uint32_t* len, int64_t* row_ptr, int64_t* chunk_tot,
                                 int64_t* chunk_off, int64_t* total, hipStream_t st) {
  const int64_t B = n_pos * ((int64_t)n_neg + 1);
  if (B <= 0) {
    launch_len_scan(len, 0, row_ptr, chunk_tot, chunk_off, total, st);
    return;
  }
  const int64_t C = candidates.n_rows;
  const int64_t stride = std::max<int64_t>(1, (C + kPivots - 1) / kPivots);
  const int np = (int)((C + stride - 1) / stride);
  hipLaunchKernelGGL(k_pair_sample_weighted, dim3(grid_for(B, kBlock)), dim3(kBlock), 0, st, pos_ctx, pos_cand, B, n_neg, excl_ptr,
                     d, C, stride, np, pos_label, neg_label, seed, contexts.row_ptr.as<int64_t>(),
                     candidates.row_ptr.as<int64_t>(), pair_ctx, pair_cand, label, len);
  launch_len_scan(len, B, row_ptr, chunk_tot, chunk_off, total, st);
}

}  // namespace fmhip
