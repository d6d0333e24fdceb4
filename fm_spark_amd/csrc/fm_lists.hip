// Resident per-context row lists: fm_lists_from_pairs' device side.  The n (context, candidate) pairs
// arrive sorted by context, then candidate (two stable radix sorts, fm_capi.hip); equal pairs are then
// neighbours and every context's pairs one run, so the lists are three one-pass kernels around a scan:
//   k_lists_flag     flag[i] = 1 where sorted pair i differs from pair i - 1 (or i = 0): the first of a run
//                    of equal pairs, i.e. one row of one list
//   launch_len_scan  off[i] = the flags before i, off[n] = the distinct pairs (fm_pairs.hip's three-phase scan)
//   k_lists_ptr      ptr[v] = off[the first sorted pair with context >= v], v in [0, U]: a binary search per
//                    offset, so a run of contexts without a pair costs its offsets alone, and ptr[U] = off[n]
//   k_lists_compact  a flagged pair i writes rows[off[i]] = its candidate row
// Integer work only, every slot with exactly one writer, no atomics: equal inputs give equal bytes.
// ptr is computed before rows exists: the host reads it back once (its copy, the longest list, and ptr[U],
// which sizes rows), then the compaction fills rows.
#include "fm_device.h"

namespace fmhip {

static_assert(kBlock == 256, "the block edges tests/test_gpu_row_lists.py places its pair and context counts at");

__global__ __launch_bounds__(kBlock) void k_lists_flag(const uint32_t* __restrict__ sctx, const uint32_t* __restrict__ scand,
                                                      int64_t n, uint32_t* __restrict__ flag) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    flag[i] = i == 0 || sctx[i] != sctx[i - 1] || scand[i] != scand[i - 1];
}

__global__ __launch_bounds__(kBlock) void k_lists_ptr(const uint32_t* __restrict__ sctx, const int64_t* __restrict__ off,
                                                     int64_t n, int64_t U, int64_t* __restrict__ ptr) {
  for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v <= U; v += (int64_t)gridDim.x * kBlock) {
    int64_t lo = 0, hi = n;  // the first i with sctx[i] >= v (n: none)
    while (lo < hi) {
      const int64_t mid = (lo + hi) / 2;
      if ((int64_t)sctx[mid] < v) lo = mid + 1;
      else hi = mid;
    }
    ptr[v] = off[lo];
  }
}

__global__ __launch_bounds__(kBlock) void k_lists_compact(const uint32_t* __restrict__ scand, const uint32_t* __restrict__ flag,
                                                         const int64_t* __restrict__ off, int64_t n,
                                                         int32_t* __restrict__ rows) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    if (flag[i]) rows[off[i]] = (int32_t)scand[i];
}

void launch_lists_offsets(const uint32_t* sctx, const uint32_t* scand, int64_t n, int64_t U, uint32_t* flag, int64_t* off,
                          int64_t* chunk_tot, int64_t* chunk_off, int64_t* total, int64_t* ptr, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(k_lists_flag, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, st, sctx, scand, n, flag);
  launch_len_scan(flag, n, off, chunk_tot, chunk_off, total, st);
  hipLaunchKernelGGL(k_lists_ptr, dim3(grid_for(U + 1, kBlock)), dim3(kBlock), 0, st, sctx, off, n, U, ptr);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_lists_compact(const uint32_t* scand, const uint32_t* flag, const int64_t* off, int64_t n, int32_t* rows,
                          hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_lists_compact, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, st, scand, flag, off, n, rows);
  FM_HIP_CHECK(hipGetLastError());
}

}  // namespace fmhip
