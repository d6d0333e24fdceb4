// Binary evaluation on the device: fm_binary_metrics / fm_evaluate_binary*'s stage.  From score[n] and
// label[n] (fp64, device) one record: the class counts, the confusion counts at the threshold score > 0,
// the log loss sum, and two_u = twice the Mann-Whitney U of the positives' scores over the negatives',
// from which AUC = two_u / (2 n_pos n_neg) -- exact (integers over the fully sorted scores, ties counted
// as half a win), not a binned approximation.
//
//   k_binary_rows    one pass over the rows, grid-stride: positive = label > 0.5, predicted positive =
//                    score > 0, the log loss term softplus(s) - y s (fm_device.h: the logistic objective's
//                    formula), per-block partials {n_pos, tp, fp, loss}; and the sort's input: the
//                    order-preserving uint64 image of s + 0.0 (negatives: all bits flipped; others: the sign
//                    bit set) split into its low word (the first sort's key) and {high word, positive flag}
//                    (its payload).  The + 0.0 makes -0.0 and +0.0 one key: they compare equal, and a
//                    (+0, -0) pair of opposite labels is a tie, not a win.
//                    16 B read, 12 B written per row.
//   sort             ascending by the 64-bit key in two stable sorts of 32-bit keys with 8-byte payloads
//                    (radix_sort_pairs64, four 9-bit passes each): by the low word, k_binary_rekey swaps the
//                    words ({high} becomes the key, {low, flag} the payload; 12 B read, 12 B written per row),
//                    then by the high word.  Each pass: 4 B + 12 B read, 12 B written per row (fm_sort.hip).
//   k_binary_flag    flag[i] = the sorted row's positive flag, for the scan (8 B read, 4 B written per row)
//   launch_len_scan  cp[i] = positives before sorted position i, cp[n] = n_pos (fm_pairs.hip's three phases)
//   k_binary_count   With A(i) = i - cp[i] the negatives before i, a run [s, e) of equal keys contributes
//                    (cp[e] - cp[s]) (A(s) + A(e)): each of its positives beats the A(s) negatives below the
//                    run twice and ties with the run's A(e) - A(s) negatives once.  The thread of a run's
//                    last element adds the run's term.  The run's first index: i itself when the element
//                    before differs (every run of a batch of distinct scores: no search), else a binary
//                    search over the sorted keys, as k_lists_ptr finds its offsets.  (The alternative, a
//                    max-scan of head indices, is a second three-kernel scan of 8-byte values over every
//                    element; at these sizes the stage is bound by its launches, and the search costs only
//                    the tails of runs of two or more, log2 n reads of keys that the sort left in cache.)
//                    A run may span blocks, tiles and scan chunks: nothing here depends on where it lies.
//   k_binary_fold    one block: the two kernels' per-block partials summed, thread t the records t,
//                    t + kBlock, ... in order, then the block's waves in order, into the 64-byte record.
//
// The integers are exact whatever the order; the loss sum runs in an order that depends on n alone.  No
// atomics: equal inputs give equal bits.  two_u <= 2 n_pos n_neg < 2^62 for n < 2^31.
// NaN scores: their keys sort above +inf (positive NaN) or below -inf (negative NaN); which, is unspecified.
#include "fm_device.h"

namespace fmhip {

namespace {

// blocks of k_binary_rows and k_binary_count at most; a larger n strides the grid (past 262 144 rows)
constexpr int kBinGrid = 1024;
constexpr int kBinRowsRec = 4;  // int64 words of a k_binary_rows partial: n_pos, tp, fp, the loss sum's bits
static_assert(kBlock == 256, "the block edge tests/test_gpu_binary.py places its row counts at");
static_assert((int64_t)kBinGrid * kBlock == 262144, "rows past which the grid is strided (tests/test_gpu_binary.py)");
static_assert(kBinaryRec * sizeof(int64_t) == 64, "the record is one 64-byte line");

__device__ __forceinline__ uint64_t score_key(double s) {
  const uint64_t b = (uint64_t)__double_as_longlong(s + 0.0);  // -0.0 + 0.0 = +0.0 (round to nearest)
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}

// the block's sum of v (xor tree within each wave, then the waves in order) on thread 0; ws: kBlock / 64
// words of LDS, free again on return
__device__ __forceinline__ int64_t block_sum_i64(int64_t v, int64_t* ws) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  int64_t t = 0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) t += ws[w];
  __syncthreads();
  return t;
}
__device__ __forceinline__ double block_sum_f64(double v, double* ws) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) t += ws[w];
  __syncthreads();
  return t;
}

__global__ __launch_bounds__(kBlock) void k_binary_rows(const double* __restrict__ score, const double* __restrict__ label,
                                                       int64_t n, uint32_t* __restrict__ key_lo, uint2* __restrict__ pay,
                                                       int64_t* __restrict__ part) {
  __shared__ int64_t wi[kBlock / 64];
  __shared__ double wd[kBlock / 64];
  int64_t n_pos = 0, tp = 0, fp = 0;
  double loss = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const double s = score[i], y = label[i];
    const bool pos = y > 0.5, hit = s > 0.0;
    n_pos += pos;
    tp += pos && hit;
    fp += !pos && hit;
    loss += softplus_d(s) - y * s;
    const uint64_t k = score_key(s);
    key_lo[i] = (uint32_t)k;
    pay[i] = make_uint2((uint32_t)(k >> 32), pos ? 1u : 0u);
  }
  n_pos = block_sum_i64(n_pos, wi);
  tp = block_sum_i64(tp, wi);
  fp = block_sum_i64(fp, wi);
  loss = block_sum_f64(loss, wd);
  if (threadIdx.x == 0) {
    int64_t* o = part + (int64_t)blockIdx.x * kBinRowsRec;
    o[0] = n_pos;
    o[1] = tp;
    o[2] = fp;
    o[3] = __double_as_longlong(loss);
  }
}

// sorted by the low word -> the second sort's input: the high word as the key, {low word, flag} as the payload
__global__ __launch_bounds__(kBlock) void k_binary_rekey(const uint32_t* __restrict__ slo, const uint2* __restrict__ spay,
                                                        int64_t n, uint32_t* __restrict__ key_hi, uint2* __restrict__ pay2) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const uint2 p = spay[i];
    key_hi[i] = p.x;
    pay2[i] = make_uint2(slo[i], p.y);
  }
}

__global__ __launch_bounds__(kBlock) void k_binary_flag(const uint2* __restrict__ sp, int64_t n, uint32_t* __restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) flag[i] = sp[i].y;
}

__device__ __forceinline__ uint64_t sorted_key(const uint32_t* __restrict__ shi, const uint2* __restrict__ sp, int64_t i) {
  return ((uint64_t)shi[i] << 32) | sp[i].x;
}

__global__ __launch_bounds__(kBlock) void k_binary_count(const uint32_t* __restrict__ shi, const uint2* __restrict__ sp,
                                                        const int64_t* __restrict__ cp, int64_t n,
                                                        int64_t* __restrict__ part) {
  __shared__ int64_t wi[kBlock / 64];
  int64_t acc = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    const uint64_t k = sorted_key(shi, sp, i);
    if (i + 1 < n && sorted_key(shi, sp, i + 1) == k) continue;  // not the last of its run
    int64_t s = i;
    if (i > 0 && sorted_key(shi, sp, i - 1) == k) {
      int64_t lo = 0, hi = i - 1;  // the first j with key[j] >= k, in [0, i - 1] (key[i - 1] == k)
      while (lo < hi) {
        const int64_t mid = (lo + hi) / 2;
        if (sorted_key(shi, sp, mid) < k) lo = mid + 1;
        else hi = mid;
      }
      s = lo;
    }
    const int64_t e = i + 1, cs = cp[s], ce = cp[e];
    acc += (ce - cs) * ((s - cs) + (e - ce));
  }
  acc = block_sum_i64(acc, wi);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

__global__ __launch_bounds__(kBlock) void k_binary_fold(const int64_t* __restrict__ rows_part, int64_t n_rows_part,
                                                       const int64_t* __restrict__ count_part, int64_t n_count_part, int64_t n,
                                                       int64_t* __restrict__ rec) {
  __shared__ int64_t wi[kBlock / 64];
  __shared__ double wd[kBlock / 64];
  int64_t n_pos = 0, tp = 0, fp = 0, two_u = 0;
  double loss = 0.0;
  for (int64_t i = threadIdx.x; i < n_rows_part; i += kBlock) {
    const int64_t* p = rows_part + i * kBinRowsRec;
    n_pos += p[0];
    tp += p[1];
    fp += p[2];
    loss += __longlong_as_double(p[3]);
  }
  for (int64_t i = threadIdx.x; i < n_count_part; i += kBlock) two_u += count_part[i];
  n_pos = block_sum_i64(n_pos, wi);
  tp = block_sum_i64(tp, wi);
  fp = block_sum_i64(fp, wi);
  two_u = block_sum_i64(two_u, wi);
  loss = block_sum_f64(loss, wd);
  if (threadIdx.x == 0) {
    rec[0] = n;
    rec[1] = n_pos;
    rec[2] = tp;
    rec[3] = fp;
    rec[4] = two_u;
    rec[5] = __double_as_longlong(loss);
    rec[6] = 0;
    rec[7] = 0;
  }
}

}  // namespace

void BinaryWork::ensure(int64_t n) {
  const size_t m = (size_t)(n > 1 ? n : 1);
  key_lo.ensure_slack(sizeof(uint32_t) * m);
  pay.ensure_slack(sizeof(uint2) * m);
  key_hi.ensure_slack(sizeof(uint32_t) * m);
  pay2.ensure_slack(sizeof(uint2) * m);
  flag.ensure_slack(sizeof(uint32_t) * m);
  cp.ensure_slack(sizeof(int64_t) * (m + 1));
  const size_t nchunks = (size_t)std::max<int64_t>(pair_scan_chunks(n), 1);
  chunk_tot.ensure_slack(sizeof(int64_t) * nchunks);
  chunk_off.ensure_slack(sizeof(int64_t) * nchunks);
  total.ensure(sizeof(int64_t));
  rows_part.ensure(sizeof(int64_t) * kBinRowsRec * kBinGrid);
  count_part.ensure(sizeof(int64_t) * kBinGrid);
  sort.ensure(n > 1 ? n : 1);
}

void launch_binary_rows(BinaryWork& w, const double* score, const double* label, int64_t n, hipStream_t st) {
  FM_REQUIRE(n >= 1 && n < (int64_t(1) << 31), "binary metrics: n out of range");
  hipLaunchKernelGGL(k_binary_rows, dim3(grid_for(n, kBlock, kBinGrid)), dim3(kBlock), 0, st, score, label, n,
                     w.key_lo.as<uint32_t>(), w.pay.as<uint2>(), w.rows_part.as<int64_t>());
  FM_HIP_CHECK(hipGetLastError());
}

void launch_binary_sort(BinaryWork& w, int64_t n, hipStream_t st) {
  const uint32_t* k1 = nullptr;
  const uint2* v1 = nullptr;
  radix_sort_pairs64(w.sort, w.key_lo.as<uint32_t>(), w.pay.as<uint2>(), n, 32, st, &k1, &v1);
  hipLaunchKernelGGL(k_binary_rekey, dim3(grid_for(n, kBlock, kBinGrid)), dim3(kBlock), 0, st, k1, v1, n,
                     w.key_hi.as<uint32_t>(), w.pay2.as<uint2>());
  FM_HIP_CHECK(hipGetLastError());
  // (the first sort's output, in the workspace, was read by the re-key: the second sort may overwrite it)
  radix_sort_pairs64(w.sort, w.key_hi.as<uint32_t>(), w.pay2.as<uint2>(), n, 32, st, &w.sorted_hi, &w.sorted_pay);
}

void launch_binary_count(BinaryWork& w, int64_t n, int64_t* rec, hipStream_t st) {
  const unsigned g = grid_for(n, kBlock, kBinGrid);
  hipLaunchKernelGGL(k_binary_flag, dim3(g), dim3(kBlock), 0, st, w.sorted_pay, n, w.flag.as<uint32_t>());
  launch_len_scan(w.flag.as<uint32_t>(), n, w.cp.as<int64_t>(), w.chunk_tot.as<int64_t>(), w.chunk_off.as<int64_t>(),
                  w.total.as<int64_t>(), st);
  hipLaunchKernelGGL(k_binary_count, dim3(g), dim3(kBlock), 0, st, w.sorted_hi, w.sorted_pay, w.cp.as<int64_t>(), n,
                     w.count_part.as<int64_t>());
  // (both kernels ran grid_for(n, kBlock, kBinGrid) blocks: that many partials each)
  hipLaunchKernelGGL(k_binary_fold, dim3(1), dim3(kBlock), 0, st, w.rows_part.as<int64_t>(), (int64_t)g,
                     w.count_part.as<int64_t>(), (int64_t)g, n, rec);
  FM_HIP_CHECK(hipGetLastError());
}

}  // namespace fmhip
