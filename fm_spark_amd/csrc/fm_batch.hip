// Batch layout kernels: the uploaded CSR image exploded into the device batch, a dataset laid out
// split after split, row selection and split rebasing; and VectorSum by key (segment-sum over
// sorted keys).
#include <algorithm>

#include "fm_device.h"

namespace fmhip {

// groupBy(key).agg(VectorSum(vec)) on sorted keys: each run summed sequentially in input
// order (the stable sort keeps it), FactorizationMachines.scala:56-67.
__global__ void k_segment_sum(const uint32_t* __restrict__ skeys, const uint32_t* __restrict__ svals, int64_t n,
                              const double* __restrict__ vecs, int32_t k, const uint32_t* __restrict__ run_index,
                              int32_t* __restrict__ out_keys, double* __restrict__ out_sums) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (i > 0 && skeys[i - 1] == skeys[i]) continue;
    const uint32_t r = run_index[i];
    out_keys[r] = (int32_t)skeys[i];
    for (int f = 0; f < k; ++f) {
      double acc = 0.0;
      for (int64_t j = i; j < n && skeys[j] == skeys[i]; ++j) acc += vecs[(int64_t)svals[j] * k + f];
      out_sums[(int64_t)r * k + f] = acc;
    }
  }
}

__global__ void k_run_index(const uint32_t* __restrict__ skeys, int64_t n, uint32_t* __restrict__ run_index,
                            int64_t* __restrict__ n_out) {
  // single block: exclusive scan of run-start flags
  __shared__ uint32_t wsum[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (int64_t b = 0; b < n; b += kBlock) {
    const int64_t i = b + threadIdx.x;
    const uint32_t f = (i < n && (i == 0 || skeys[i - 1] != skeys[i])) ? 1u : 0u;
    uint32_t v = f;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = __shfl_up(v, o);
      if (lane >= o) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    uint32_t wpre = 0, tot = 0;
    for (int w = 0; w < kBlock / 64; ++w) {
      wpre += w < wave ? wsum[w] : 0u;
      tot += wsum[w];
    }
    if (i < n) run_index[i] = carry + wpre + v - f;
    carry += tot;
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_out = carry;
}
// One team of 16 lanes per sample: its entries get {sample, x}, x = 1 unless the id's bit 31 says
// the value follows in the row's run of compact values (xoff); col (bit 31 cleared), label and
// row_ptr are copied alongside (grid-stride, the same pass).
__global__ __launch_bounds__(kBlock) void k_explode(const int64_t* __restrict__ rp_in, const double* __restrict__ lab_in,
                                                   const int32_t* __restrict__ xoff, const uint32_t* __restrict__ col_in,
                                                   const float* __restrict__ x_in, int64_t B, int64_t* __restrict__ rp,
                                                   double* __restrict__ lab, uint32_t* __restrict__ col,
                                                   uint2* __restrict__ ent, float* __restrict__ xs) {
  constexpr int T = 16;
  const int tl = threadIdx.x % T;
  const int lane = threadIdx.x & 63;
  const uint64_t team_bits = 0xFFFFull << (lane & ~(T - 1));
  const uint64_t below = team_bits & ((1ull << lane) - 1ull);
  const int64_t gtid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = gtid; i <= B; i += nthreads) rp[i] = rp_in[i];
  for (int64_t i = gtid; i < B; i += nthreads) lab[i] = lab_in[i];
  for (int64_t s = gtid / T; s < B; s += nthreads / T) {
    const int64_t e0 = rp_in[s], e1 = rp_in[s + 1];
    int64_t xo = xoff[s];
    for (int64_t eb = rp_in[s]; eb < e1; eb += T) {  // the team's lanes take the same trips
      const int64_t e = eb + tl;
      const uint32_t c = e < e1 ? col_in[e] : 0u;
      const bool valued = (c >> 31) != 0u;
      const uint64_t m = __ballot(valued);
      const float x = valued ? x_in[xo + __popcll(m & below)] : 1.0f;
      xo += __popcll(m & team_bits);
      if (e < e1) {
        col[e] = c & 0x7FFFFFFFu;
        ent[e] = make_uint2((uint32_t)s, __float_as_uint(x));
        xs[e] = x;
      }
    }
  }
}

// fm_batch_layout_splits: the cached dfData in its own row order (the uploaded image, as k_explode
// reads it) -> the dataset laid out split after split (FactorizationMachinesSGD.scala:93, 111-112),
// in one pass: laid-out row s is source row order[s].  One team of 16 lanes per laid-out row finds
// its split (the binary search of k_split_rebase), reads the source row's ids straight from the
// image -- a valued entry's x at xoff[row] + its rank among the row's valued entries (team ballot,
// carried across the row's 16-entry trips, as k_explode) -- and writes col, xs, ent = {s - its
// split's first row, x bits}, label, row_ptr (rp_in, computed by the host) and the split's rebased
// row_ptr slots in split_rp (zeroed beforehand: an empty split's one slot stays 0).  What
// k_explode + k_select_rows + k_split_rebase would write, without the exploded source between them.
__global__ __launch_bounds__(kBlock) void k_layout_splits(const int64_t* __restrict__ src_rp, const double* __restrict__ src_lab,
                                                         const int32_t* __restrict__ xoff, const uint32_t* __restrict__ col_in,
                                                         const float* __restrict__ x_in, const int64_t* __restrict__ order,
                                                         const int64_t* __restrict__ rp_in,
                                                         const int64_t* __restrict__ split_rows, int32_t n_splits, int64_t B,
                                                         int64_t* __restrict__ rp, double* __restrict__ lab,
                                                         uint32_t* __restrict__ col, uint2* __restrict__ ent,
                                                         float* __restrict__ xs, int64_t* __restrict__ split_rp) {
  constexpr int T = 16;
  const int tl = threadIdx.x % T;
  const int lane = threadIdx.x & 63;
  const uint64_t team_bits = 0xFFFFull << (lane & ~(T - 1));
  const uint64_t below = team_bits & ((1ull << lane) - 1ull);
  const int64_t gtid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  if (gtid == 0) rp[B] = rp_in[B];
  for (int64_t s = gtid / T; s < B; s += nthreads / T) {
    int lo = 0, hi = n_splits;  // the split holding row s: split_rows[lo] <= s < split_rows[lo + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) / 2;
      if (split_rows[mid] <= s) lo = mid;
      else hi = mid;
    }
    const int64_t r0 = split_rows[lo], eb = rp_in[r0];
    const int64_t e0 = rp_in[s], e1 = rp_in[s + 1];
    const int64_t src = order[s];
    const int64_t d = src_rp[src] - e0;  // source entry of laid-out entry e: e + d
    int64_t xo = xoff[src];
    if (tl == 0) {
      rp[s] = e0;
      lab[s] = src_lab[src];
      split_rp[s + lo] = e0 - eb;
      if (s + 1 == split_rows[lo + 1]) split_rp[s + 1 + lo] = e1 - eb;
    }
    for (int64_t eb16 = e0; eb16 < e1; eb16 += T) {  // the team's lanes take the same trips
      const int64_t e = eb16 + tl;
      const uint32_t c = e < e1 ? col_in[e + d] : 0u;
      const bool valued = (c >> 31) != 0u;
      const uint64_t m = __ballot(valued);
      const float x = valued ? x_in[xo + __popcll(m & below)] : 1.0f;
      xo += __popcll(m & team_bits);
      if (e < e1) {
        col[e] = c & 0x7FFFFFFFu;
        ent[e] = make_uint2((uint32_t)(s - r0), __float_as_uint(x));
        xs[e] = x;
      }
    }
  }
}

// fm_batch_from_rows: output row s is row rows[s] of a resident dataset (the randomSplit split of
// the cached dfData, FactorizationMachinesSGD.scala:93, 111-112).  One team of 16 lanes per output
// row copies the source row's ids and fp32 x (8 B per entry, contiguous) and writes the exploded
// {s, x} entries; row_ptr (computed by the host from the dataset's row_ptr) and the labels are
// written alongside (grid-stride, the same pass).
__global__ __launch_bounds__(kBlock) void k_select_rows(const int64_t* __restrict__ src_rp, const uint32_t* __restrict__ src_col,
                                                       const float* __restrict__ src_xs, const double* __restrict__ src_lab,
                                                       const int64_t* __restrict__ rows, const int64_t* __restrict__ rp_in,
                                                       int64_t B, int64_t* __restrict__ rp, double* __restrict__ lab,
                                                       uint32_t* __restrict__ col, uint2* __restrict__ ent,
                                                       float* __restrict__ xs) {
  constexpr int T = 16;
  const int tl = threadIdx.x % T;
  const int64_t gtid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t i = gtid; i <= B; i += nthreads) rp[i] = rp_in[i];
  for (int64_t i = gtid; i < B; i += nthreads) lab[i] = src_lab[rows[i]];
  for (int64_t s = gtid / T; s < B; s += nthreads / T) {
    const int64_t e0 = rp_in[s], e1 = rp_in[s + 1];
    const int64_t d = src_rp[rows[s]] - e0;  // source entry of output entry e: e + d
    for (int64_t e = e0 + tl; e < e1; e += T) {
      const uint32_t c = src_col[e + d];
      const float x = src_xs[e + d];
      col[e] = c;
      xs[e] = x;
      ent[e] = make_uint2((uint32_t)s, __float_as_uint(x));
    }
  }
}

// fm_batch_create_splits: a dataset laid out split after split (split_rows [n_splits + 1] row offsets,
// the randomSplit splits of the cached dfData in iteration order, FactorizationMachinesSGD.scala:93,
// 111-112).  Each split's rows get their own row_ptr, rebased to the split's first entry, at
// split_rp[split_rows[s] + s ..= split_rows[s + 1] + s] (zeroed beforehand, so an empty split's one
// slot is 0), and each entry's sample index becomes relative to its split's first row: a split is
// then a mini-batch in place (fm_batch_split_view), with no gather.  One team of 16 lanes per row.
__global__ __launch_bounds__(kBlock) void k_split_rebase(const int64_t* __restrict__ rp, const int64_t* __restrict__ split_rows,
                                                        int32_t n_splits, int64_t B, uint2* __restrict__ ent,
                                                        int64_t* __restrict__ split_rp) {
  constexpr int T = 16;
  const int tl = threadIdx.x % T;
  const int64_t gtid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * kBlock;
  for (int64_t s = gtid / T; s < B; s += nthreads / T) {
    int lo = 0, hi = n_splits;  // the split holding row s: split_rows[lo] <= s < split_rows[lo + 1]
    while (hi - lo > 1) {
      const int mid = (lo + hi) / 2;
      if (split_rows[mid] <= s) lo = mid;
      else hi = mid;
    }
    const int64_t r0 = split_rows[lo], eb = rp[r0];
    const int64_t e0 = rp[s], e1 = rp[s + 1];
    if (tl == 0) {
      split_rp[s + lo] = e0 - eb;
      if (s + 1 == split_rows[lo + 1]) split_rp[s + 1 + lo] = e1 - eb;
    }
    for (int64_t e = e0 + tl; e < e1; e += T) ent[e].x = (uint32_t)(s - r0);
  }
}
void launch_explode(const CsrImage& in, int64_t B, int64_t N, BatchDev& dst, hipStream_t st) {
  (void)N;
  hipLaunchKernelGGL(k_explode, dim3(grid_for(std::max<int64_t>(B, 1) * 16, kBlock, 256 * 8)), dim3(kBlock), 0, st,
                     in.row_ptr, in.label, in.xoff, in.col, in.x, B, dst.row_ptr.as<int64_t>(), dst.label.as<double>(),
                     dst.col.as<uint32_t>(), dst.ent.as<uint2>(), dst.xs.as<float>());
  FM_HIP_CHECK(hipGetLastError());
}

void launch_layout_splits(const CsrImage& src, const int64_t* order, const int64_t* row_ptr_in, const int64_t* split_rows,
                          int32_t n_splits, int64_t B, BatchDev& dst, int64_t* split_rp, hipStream_t st) {
  FM_HIP_CHECK(hipMemsetAsync(split_rp, 0, sizeof(int64_t) * (B + n_splits), st));
  hipLaunchKernelGGL(k_layout_splits, dim3(grid_for(std::max<int64_t>(B, 1) * 16, kBlock, 256 * 8)), dim3(kBlock), 0, st,
                     src.row_ptr, src.label, src.xoff, src.col, src.x, order, row_ptr_in, split_rows, n_splits, B,
                     dst.row_ptr.as<int64_t>(), dst.label.as<double>(), dst.col.as<uint32_t>(), dst.ent.as<uint2>(),
                     dst.xs.as<float>(), split_rp);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_select_rows(const BatchDev& src, const int64_t* rows, const int64_t* row_ptr_in, int64_t B, BatchDev& dst,
                        hipStream_t st) {
  hipLaunchKernelGGL(k_select_rows, dim3(grid_for(std::max<int64_t>(B, 1) * 16, kBlock, 256 * 8)), dim3(kBlock), 0, st,
                     src.row_ptr.as<int64_t>(), src.col.as<uint32_t>(), src.xs.as<float>(), src.label.as<double>(), rows,
                     row_ptr_in, B, dst.row_ptr.as<int64_t>(), dst.label.as<double>(), dst.col.as<uint32_t>(),
                     dst.ent.as<uint2>(), dst.xs.as<float>());
  FM_HIP_CHECK(hipGetLastError());
}

void launch_split_rebase(const BatchDev& b, const int64_t* split_rows, int32_t n_splits, int64_t* split_rp,
                         hipStream_t st) {
  const int64_t B = b.n_rows;
  FM_HIP_CHECK(hipMemsetAsync(split_rp, 0, sizeof(int64_t) * (B + n_splits), st));
  if (B == 0) return;
  hipLaunchKernelGGL(k_split_rebase, dim3(grid_for(B * 16, kBlock, 256 * 8)), dim3(kBlock), 0, st,
                     b.row_ptr.as<int64_t>(), split_rows, n_splits, B, b.ent.as<uint2>(), split_rp);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_segment_sum(const uint32_t* skeys, const uint32_t* svals, int64_t n, const double* vecs, int32_t k,
                        uint32_t* run_index, int32_t* out_keys, double* out_sums, int64_t* n_out_dev,
                        hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_run_index, dim3(1), dim3(kBlock), 0, st, skeys, n, run_index, n_out_dev);
  hipLaunchKernelGGL(k_segment_sum, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, st, skeys, svals, n, vecs, k,
                     run_index, out_keys, out_sums);
  FM_HIP_CHECK(hipGetLastError());
}

}  // namespace fmhip
