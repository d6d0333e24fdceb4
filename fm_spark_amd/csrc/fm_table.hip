// Table utilities of the FM model on the device: seeded init (createInitialModel), load, gather,
// reset, flush (pending L1 applied to every row) and the present-row count.  The seeded draw
// (gauss_draw) and the row arithmetic: fm_device.h.
#include "fm_device.h"

namespace fmhip {

// ---------------------------------------------------------------- table utilities
// ids != nullptr: the listed ids (those this shard owns); else every id in [id_begin, id_begin + n)
// that this shard owns, walked slot by slot (i = the i-th owned id of the range)
__global__ void k_init_random(TableView T, const int32_t* __restrict__ ids, int64_t n, int64_t id_begin,
                              uint64_t seed, double sd, int32_t epoch, double cumE) {
  const int64_t R = T.shard_count;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t id;
    if (ids) {
      id = (int64_t)ids[i];
      if (id % R != T.shard_index) continue;
    } else {
      const int64_t first = id_begin + ((T.shard_index - id_begin % R) % R + R) % R;  // first owned id >= id_begin
      id = first + i * R;
    }
    const int64_t slot = id / R;
    if (slot >= T.rows) continue;
    for (int f = 0; f < T.kp; ++f) T.v(slot)[f] = f < T.k ? gauss_draw(seed, id, f, sd) : 0.f;
    store_hdr(T, slot, RowHdr{gauss_draw(seed, id, -1, sd), epoch, cumE});
  }
}

// createInitialModel (SGD.scala:218-252) from the data itself: every id of the batch's entries
// that this context owns and that is absent gets the seeded draw of k_init_random.  The draw is a
// function of (seed, id, factor) only, so no distinct pass is needed: entries of one id that race
// write identical bytes, and rows already present are kept.
__global__ void k_init_entries(TableView T, const uint32_t* __restrict__ col, int64_t n, uint64_t seed, double sd,
                               int32_t epoch, double cumE) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t id = (int64_t)col[i];
    if (id % T.shard_count != T.shard_index) continue;
    const int64_t slot = id / T.shard_count;
    if (slot >= T.rows || T.hdr(slot)->t >= 0) continue;
    for (int f = 0; f < T.kp; ++f) T.v(slot)[f] = f < T.k ? gauss_draw(seed, id, f, sd) : 0.f;
    store_hdr(T, slot, RowHdr{gauss_draw(seed, id, -1, sd), epoch, cumE});
  }
}

__global__ void k_load_rows(TableView T, const int32_t* __restrict__ ids, int64_t n, const double* __restrict__ w,
                            const double* __restrict__ V, int32_t epoch, double cumE) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t id = ids[i];
    if (id % T.shard_count != T.shard_index) continue;
    const int64_t slot = id / T.shard_count;
    if (slot >= T.rows) continue;
    for (int f = 0; f < T.kp; ++f) T.v(slot)[f] = f < T.k ? (float)V[i * T.k + f] : 0.f;
    store_hdr(T, slot, RowHdr{(float)w[i], epoch, cumE});
  }
}

// Rows by feature id (owned by this shard), brought current (pending L1 applied) without writing
// the table: the model Datasets queried by id (Strength / FactorizedInteraction, Model.scala:281,289)
__global__ void k_gather_rows(TableView T, const int32_t* __restrict__ ids, int64_t n, double cumE,
                              double* __restrict__ w_out, double* __restrict__ V_out, int8_t* __restrict__ present) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t slot = (int64_t)ids[i] / T.shard_count;
    const RowHdr h = *T.hdr(slot);
    const bool pr = h.t >= 0;
    const double a = pr ? cumE - h.cum : 0.0;
    present[i] = pr ? 1 : 0;
    w_out[i] = pr ? (double)(a > 0.0 ? shrink_f(h.w, a) : h.w) : 0.0;
    const float* v = T.v(slot);
    for (int f = 0; f < T.k; ++f) V_out[i * T.k + f] = pr ? (double)(a > 0.0 ? shrink_f(v[f], a) : v[f]) : 0.0;
  }
}

__global__ void k_table_reset(TableView T) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < T.rows; i += (int64_t)gridDim.x * blockDim.x)
    store_hdr(T, i, RowHdr{0.f, -1, 0.0});
}

__global__ void k_flush(TableView T, int32_t epoch, double cumE) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < T.rows; i += (int64_t)gridDim.x * blockDim.x) {
    RowHdr h = (*T.hdr(i));
    if (h.t < 0) continue;
    const double a = cumE - h.cum;
    if (a > 0.0) {
      h.w = shrink_f(h.w, a);
      for (int f = 0; f < T.kp; ++f) T.v(i)[f] = shrink_f(T.v(i)[f], a);
    }
    h.t = epoch;
    h.cum = cumE;
    store_hdr(T, i, h);
  }
}

__global__ void k_count_present(TableView T, unsigned long long* out) {
  unsigned long long c = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < T.rows; i += (int64_t)gridDim.x * blockDim.x)
    c += (*T.hdr(i)).t >= 0 ? 1ull : 0ull;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, c);
}
void launch_init_random(const TableView& T, const int32_t* ids, int64_t n, int64_t id_begin, uint64_t seed,
                        double sd, int32_t epoch, double cumE, hipStream_t st) {
  if (n <= 0) return;
  if (!ids) {  // a range: only the ids this shard owns
    const int64_t R = T.shard_count, end = id_begin + n;
    const int64_t first = id_begin + ((T.shard_index - id_begin % R) % R + R) % R;
    n = first < end ? (end - first + R - 1) / R : 0;
    if (n <= 0) return;
  }
  hipLaunchKernelGGL(k_init_random, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, st, T, ids, n, id_begin, seed, sd,
                     epoch, cumE);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_init_entries(const TableView& T, const uint32_t* col, int64_t n, uint64_t seed, double sd, int32_t epoch,
                         double cumE, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_init_entries, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, st, T, col, n, seed, sd, epoch,
                     cumE);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_load_rows(const TableView& T, const int32_t* ids, int64_t n, const double* w, const double* V,
                      int32_t epoch, double cumE, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_load_rows, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, st, T, ids, n, w, V, epoch, cumE);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_gather_rows(const TableView& T, const int32_t* ids, int64_t n, double cumE, double* w, double* V,
                        int8_t* present, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_gather_rows, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, st, T, ids, n, cumE, w, V, present);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_table_reset(const TableView& T, hipStream_t st) {
  if (T.rows <= 0) return;
  FM_HIP_CHECK(hipMemsetAsync(T.rec, 0, sizeof(float) * (size_t)T.rows * T.stride, st));
  hipLaunchKernelGGL(k_table_reset, dim3(grid_for(T.rows, kBlock)), dim3(kBlock), 0, st, T);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_flush(const TableView& T, int32_t epoch, double cumE, hipStream_t st) {
  if (T.rows <= 0) return;
  hipLaunchKernelGGL(k_flush, dim3(grid_for(T.rows, kBlock)), dim3(kBlock), 0, st, T, epoch, cumE);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_count_present(const TableView& T, int64_t* out, hipStream_t st) {
  FM_HIP_CHECK(hipMemsetAsync(out, 0, sizeof(int64_t), st));
  if (T.rows <= 0) return;
  hipLaunchKernelGGL(k_count_present, dim3(grid_for(T.rows, kBlock)), dim3(kBlock), 0, st, T,
                     reinterpret_cast<unsigned long long*>(out));
  FM_HIP_CHECK(hipGetLastError());
}

}  // namespace fmhip
