// (context, candidate) pair batches: fm_batch_from_pairs' and fm_batch_sample_pairs' device side.
//   k_pair_rows    the gather both calls share: output row s = the entries of row pair_ctx[s] of the
//                  contexts followed by those of row pair_cand[s] of the candidates
//   k_pair_sample  the sampled call's pairs: each positive, then its n_neg drawn candidate rows, with
//                  every output row's label and length
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
// gather (copy-stream order) and no event or host wait protects the scratch between calls.
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

// inclusive scan of v over the block's threads (NW waves; ws: NW int64 of LDS); *total = the block's sum
template <int NW>
__device__ __forceinline__ int64_t block_scan_incl(int64_t v, int64_t* ws, int64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int64_t t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  if (lane == 63) ws[wave] = v;
  __syncthreads();
  int64_t wpre = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    wpre += w < wave ? ws[w] : 0;
    tot += ws[w];
  }
  __syncthreads();  // ws is free for the next call
  *total = tot;
  return v + wpre;
}

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
