// The AdaGrad update stage of the single-table step for gfx950 (MI355X): fm_config.optimizer ==
// FM_OPT_ADAGRAD.  It takes launch_segment_update's place in the step (fm_capi.hip step_impl): the same
// sorted view, S records and {r, yh} pairs in, the table and the accumulator rows updated, stats[3]
// closed.  The SGD kernels (fm_update.hip) are not touched and an SGD context launches none of these.
//
// Per touched row, with g the run's fp64 gradient sum (fm_update.hip: g_V[f] = A[f] - v_cur[f] b,
// A = sum S (x r), b = sum x^2 r; g_w = sum (x - 1) yh + r) and gh = g / m:
//     G' = G + gh^2        v' = S_lam(v_cur - eta gh / sqrt(G'))        G <- (float) G'
// in fp64, v' rounded once.  The soft threshold is NOT scaled by the adaptive rate: the lazy L1 stays
// one global `cum`, so the forward's catch-up, predict, rank and export are unchanged (include/fm_hip.h).
//
// The work is cut by runs, not by position.  A run of equal keys is cut into pieces of kAdaPiece entries
// counted from the run's first entry, so every sum's order depends on the run alone -- the same run at
// another offset of the batch, prepared or sorted inline, gives the same bits.  No float atomics.
//   k_ada_flag    one thread per sorted entry: 1 where a piece begins (a run's first entry, and every
//                 kAdaPiece-th after it: the entries of a wave at least kAdaPiece deep in a run share one
//                 lower bound over the keys for the run's start).  Per-block counts of run heads (the distinct ids), and
//                 the heads of runs longer than one piece appended to a list (an integer atomic counter:
//                 the list's order varies, no sum depends on it).
//   launch_len_scan (fm_pairs.hip) the flags' exclusive scan: off[i] = pieces before entry i, total = P.
//   k_ada_piece   one lane group of Q lanes per piece (kp <= 16: 4 lanes, a float4 column quad each; wider
//                 rows 16 lanes and up to 4 quads per lane).  Piece j finds its first entry by binary
//                 search over the scanned offsets, then walks its entries in order, four entries' keys,
//                 payloads, S quads and {r, yh} loaded ahead, into fp64 {A[kp], b, g_w}.  A piece that is
//                 its whole run applies the update at once (the row, its header and its accumulator row
//                 were requested before the walk); any other leaves its partial in slot
//                 2 (first entry / kAdaPiece) + (heads its run): full pieces lie kAdaPiece apart, so a window
//                 of kAdaPiece positions holds at most one run's last piece and one run's first.
//   k_ada_fold    one lane group per listed run: its pieces' partials summed in piece order (the piece
//                 count by a doubling search over the keys, so the partial loads do not wait on each
//                 other), then the same row update.  Block 0 closes the step as k_segment_combine's block 0
//                 does -- the loss partials in that kernel's order, so a first AdaGrad step reports the
//                 bits of an SGD step's loss.
// Every row and accumulator row is read once and written once, when its run closes; the header's 64-B
// granule is completed (hdr_span) and the accumulator row [kp + 4] = {G_V, G_w, 0, 0, 0} leaves in whole
// 16-byte stores.
#include <algorithm>
#include <type_traits>

#include "fm_device.h"

namespace fmhip {

namespace {

constexpr int kAdaPiece = 128;  // entries per piece
constexpr int kAdaAhead = 4;    // entries a lane group loads per round of its walk
constexpr int kStatLd = 8;      // the closing block's loads in flight per thread (k_segment_combine's)

struct AdaArgs {
  TableView T;
  float* G;               // [rows][kp + 4] accumulators
  const uint32_t* skeys;  // sorted feature slots
  const uint2* sents;     // their entries {sample, x bits}
  int64_t N;
  const float* S;
  const float2* yl;
  int64_t s_stride, yl_stride;
  StepParams p;
  const int64_t* off;    // [N + 1] pieces before each entry
  const int64_t* total;  // [1] P
  double* part;          // [2 ceil(N / kAdaPiece)][kp + 2] = [g_w | A (kp) | b]
  int64_t* hot;          // heads of the runs of several pieces
  unsigned long long* hot_n;  // their count (this step's counter)
};

// ------------------------------------------------------------------------------- piece flags
__global__ __launch_bounds__(kBlock) void k_ada_flag(const uint32_t* __restrict__ skeys, int64_t N, uint32_t* __restrict__ flag,
                                                     uint32_t* __restrict__ ucnt, int64_t* __restrict__ hot,
                                                     unsigned long long* __restrict__ hot_n,
                                                     unsigned long long* __restrict__ hot_n_next) {
  __shared__ uint32_t wcnt[kBlock / 64];
  if (blockIdx.x == 0 && threadIdx.x == 0) *hot_n_next = 0ull;  // the next step's counter (the steps alternate)
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = i < N;
  const uint32_t key = in ? skeys[i] : 0u;
  const bool head = in && (i == 0 || skeys[i - 1] != key);
  const bool deep = in && !head && i >= kAdaPiece && skeys[i - kAdaPiece] == key;
  // One search per key and wave, not per entry: the first lane of every stretch of equal keys (the keys are
  // sorted, so a stretch is contiguous) finds the run's first entry -- itself if it heads the run, else a lower
  // bound over the keys before it -- and its stretch reads the result.  The loop is wave-uniform.
  const uint32_t up = __shfl_up(key, 1);
  const bool lead = in && (lane == 0 || up != key);
  const uint64_t leads = __ballot(lead), deeps = __ballot(deep);
  const uint64_t upto = lane == 63 ? ~0ull : ((2ull << lane) - 1);
  const int leader = 63 - __clzll((long long)((leads & upto) | 1ull));
  // the stretch of a leader ends before the next leader: does it hold an entry that needs the run's start?
  const uint64_t above = lane == 63 ? 0ull : (leads >> (lane + 1)) << (lane + 1);
  const uint64_t mine = above ? ((1ull << (__ffsll((long long)above) - 1)) - 1) & ~(upto >> 1) : ~(upto >> 1);
  int64_t lo = i, hi = i;
  if (lead && !head && (deeps & mine)) lo = 0;
  while (__any(lo < hi)) {
    if (lo < hi) {
      const int64_t mid = (lo + hi) / 2;
      if (skeys[mid] < key) lo = mid + 1;
      else hi = mid;
    }
  }
  const int64_t start = __shfl(lo, leader);
  if (in) {
    flag[i] = head || (deep && (i - start) % kAdaPiece == 0);
    if (head && i + kAdaPiece < N && skeys[i + kAdaPiece] == key) hot[atomicAdd(hot_n, 1ull)] = i;
  }
  const uint32_t c = (uint32_t)__popcll(__ballot(head));
  if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) t += wcnt[w];
    ucnt[blockIdx.x] = t;
  }
}

// ------------------------------------------------------------------------------- the row update
// One lane's share of a row as it was stored: NF V quads and their accumulator quads, the header and the
// accumulator row's last quad {G_w, 0, 0, 0}.
template <int NF>
struct AdaRow {
  float4 v[NF], g[NF], h, gw;
};
template <int Q, int NF>
__device__ __forceinline__ void ada_load_row(const AdaArgs& a, uint32_t slot, int q, AdaRow<NF>& r) {
  const int kp = a.T.kp;
  const float* rec = a.T.v(slot);
  const float* acc = a.G + (int64_t)slot * (kp + 4);
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    const int c = 4 * (q + Q * n);
    r.v[n] = c < kp ? *reinterpret_cast<const float4*>(rec + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    r.g[n] = c < kp ? *reinterpret_cast<const float4*>(acc + c) : make_float4(1.f, 1.f, 1.f, 1.f);
  }
  r.h = *reinterpret_cast<const float4*>(rec + kp);
  r.gw = *reinterpret_cast<const float4*>(acc + kp);
}

// G' = G + gh^2 and the step from v: S_lam(v - eta gh / sqrt(G')), fp64, each rounded once
__device__ __forceinline__ float ada_coord(float v, double g, float& G, const StepParams& p) {
  const double gh = g / p.m;
  const double Gn = (double)G + gh * gh;
  G = (float)Gn;
  return (float)shrink_d((double)v - p.eta * gh / sqrt(Gn), p.lam);
}

// The run's sums applied to its row.  The row is brought current as the SGD update brings it (pending_l1
// and the fp32 soft threshold; an absent row counts as zero with nothing pending) and leaves with next_hdr.
template <int Q, int NF>
__device__ __forceinline__ void ada_apply(const AdaArgs& a, uint32_t slot, int q, const AdaRow<NF>& r, const double* A,
                                          double b, double gw) {
  const int kp = a.T.kp;
  const RowHdr h = *reinterpret_cast<const RowHdr*>(&r.h);
  const bool present = h.t >= 0;
  const float acf = present ? pending_l1(h, a.p) : 0.f;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float* rec = a.T.v(slot);
  float* acc = a.G + (int64_t)slot * (kp + 4);
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    const int c = 4 * (q + Q * n);
    if (c >= kp) continue;
    const QuadGrad qg = quad_grad(present ? r.v[n] : zero, acf, A + 4 * n, b);  // v_cur and g = A - v_cur b
    float4 G = r.g[n], o;
    o.x = ada_coord(qg.v.x, qg.g0, G.x, a.p);
    o.y = ada_coord(qg.v.y, qg.g1, G.y, a.p);
    o.z = ada_coord(qg.v.z, qg.g2, G.z, a.p);
    o.w = ada_coord(qg.v.w, qg.g3, G.w, a.p);
    st_row4(rec + c, o);
    st_row4(acc + c, G);
  }
  float Gw = r.gw.x;
  const float w_new = ada_coord(present ? shrink1f(h.w, acf) : 0.f, gw, Gw, a.p);
  // the header and the zero pad of its 64-B granule, written whole by the group's lanes
  const int span = hdr_span(kp);
  for (int i = 4 * q; i < span; i += 4 * Q) {
    float4 hv = zero;
    if (i == 0) {
      const RowHdr o = next_hdr(w_new, a.p);
      hv = *reinterpret_cast<const float4*>(&o);
    }
    st_row4(rec + kp + i, hv);
  }
  if (q == 0) st_row4(acc + kp, make_float4(Gw, 0.f, 0.f, 0.f));
}

__device__ __forceinline__ int64_t ada_slot(int64_t first, bool head) { return 2 * (first / kAdaPiece) + (head ? 1 : 0); }

// ------------------------------------------------------------------------------- pieces
template <int Q, int NF>
__global__ __launch_bounds__(kBlock) void k_ada_piece(AdaArgs a) {
  constexpr int C = 4 * NF, NG = kBlock / Q;
  const int q = threadIdx.x % Q;
  const int kp = a.T.kp;
  const int64_t N = a.N, P = a.total[0];
  for (int64_t j = (int64_t)blockIdx.x * NG + threadIdx.x / Q; j < P; j += (int64_t)gridDim.x * NG) {
    // the piece's first entry: the first i with off[i + 1] > j
    int64_t lo = 0, hi = N - 1;
    while (lo < hi) {
      const int64_t mid = (lo + hi) / 2;
      if (a.off[mid + 1] > j) hi = mid;
      else lo = mid + 1;
    }
    const int64_t first = lo;
    const uint32_t key = a.skeys[first];
    const bool head = first == 0 || a.skeys[first - 1] != key;
    const int64_t lim = first + kAdaPiece < N ? first + kAdaPiece : N;
    // the piece is its whole run (k_ada_flag's test): only then is the row read here, in flight during the walk;
    // the row of a run of several pieces is read by k_ada_fold alone
    const bool whole = head && !(lim < N && lim == first + kAdaPiece && a.skeys[lim] == key);
    AdaRow<NF> row;
    if (whole) ada_load_row<Q, NF>(a, key, q, row);
    double A[C];
#pragma unroll
    for (int c = 0; c < C; ++c) A[c] = 0.0;
    double b = 0.0, gw = 0.0;
    int64_t e = first;
    bool more = true;
    while (more) {
      uint2 en[kAdaAhead];
      bool ok[kAdaAhead];
#pragma unroll
      for (int u = 0; u < kAdaAhead; ++u) {
        const int64_t pos = e + u < N ? e + u : N - 1;  // clamped: issued together
        ok[u] = a.skeys[pos] == key;
        en[u] = a.sents[pos];
      }
      float4 Sq[kAdaAhead][NF];
      float2 y[kAdaAhead];
#pragma unroll
      for (int u = 0; u < kAdaAhead; ++u) {
        ok[u] = ok[u] && e + u < lim;  // the keys are sorted: the first false ends the piece
        const int64_t s = (int64_t)en[u].x;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
          const int c = 4 * (q + Q * n);
          Sq[u][n] = (ok[u] && c < kp) ? *reinterpret_cast<const float4*>(a.S + s * a.s_stride + c)
                                       : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        y[u] = ok[u] ? a.yl[s * a.yl_stride] : make_float2(0.f, 0.f);
      }
#pragma unroll
      for (int u = 0; u < kAdaAhead; ++u) {
        if (!ok[u]) {
          more = false;
          break;
        }
        // t = x r, x^2 r and g_w = (x - 1) yh + r, as the SGD update forms them
        const double xd = (double)__uint_as_float(en[u].y), rj = (double)y[u].x, yh = (double)y[u].y;
        const double t = xd * rj;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
          A[4 * n + 0] = fma((double)Sq[u][n].x, t, A[4 * n + 0]);
          A[4 * n + 1] = fma((double)Sq[u][n].y, t, A[4 * n + 1]);
          A[4 * n + 2] = fma((double)Sq[u][n].z, t, A[4 * n + 2]);
          A[4 * n + 3] = fma((double)Sq[u][n].w, t, A[4 * n + 3]);
        }
        b += (xd * xd) * rj;
        gw += (xd - 1.0) * yh + rj;
        ++e;
      }
    }
    if (whole) {
      ada_apply<Q, NF>(a, key, q, row, A, b, gw);
    } else {
      double* pr = a.part + ada_slot(first, head) * (int64_t)(kp + 2);
#pragma unroll
      for (int n = 0; n < NF; ++n) {
        const int c = 4 * (q + Q * n);
        if (c < kp) {
          pr[1 + c + 0] = A[4 * n + 0];
          pr[1 + c + 1] = A[4 * n + 1];
          pr[1 + c + 2] = A[4 * n + 2];
          pr[1 + c + 3] = A[4 * n + 3];
        }
      }
      if (q == 0) {
        pr[0] = gw;
        pr[kp + 1] = b;
      }
    }
  }
}

// ------------------------------------------------------------------------------- fold and close
template <int Q, int NF>
__global__ __launch_bounds__(kBlock) void k_ada_fold(AdaArgs a, const double2* __restrict__ loss_part, int64_t n_loss_blocks,
                                                     const uint32_t* __restrict__ ucnt, int64_t n_ucnt,
                                                     double* __restrict__ stats_out) {
  constexpr int C = 4 * NF, NG = kBlock / Q;
  const int tid = threadIdx.x;
  if (blockIdx.x == 0) {
    // k_segment_combine's block 0, sum for sum: thread t takes the partials t, t + kBlock, ... in order
    // (kStatLd loads at a time from clamped addresses), then the block's tree
    __shared__ double rl[kBlock], rc[kBlock], ru[kBlock];
    double l = 0.0, c = 0.0, u = 0.0;
    for (int64_t i0 = tid; i0 < n_loss_blocks; i0 += kStatLd * kBlock) {
      double2 v[kStatLd];
#pragma unroll
      for (int j = 0; j < kStatLd; ++j) {
        const int64_t i = i0 + j * kBlock;
        v[j] = loss_part[i < n_loss_blocks ? i : n_loss_blocks - 1];
      }
#pragma unroll
      for (int j = 0; j < kStatLd; ++j) {
        const bool in = i0 + j * kBlock < n_loss_blocks;
        l += in ? v[j].x : 0.0;
        c += in ? v[j].y : 0.0;
      }
    }
    for (int64_t i = tid; i < n_ucnt; i += kBlock) u += (double)ucnt[i];  // whole numbers: exact in any order
    rl[tid] = l;
    rc[tid] = c;
    ru[tid] = u;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
      if (tid < o) {
        rl[tid] += rl[tid + o];
        rc[tid] += rc[tid + o];
        ru[tid] += ru[tid + o];
      }
      __syncthreads();
    }
    if (tid == 0) {
      stats_out[0] = rl[0];
      stats_out[1] = rc[0];
      stats_out[2] = ru[0];
    }
  }
  const int q = tid % Q;
  const int kp = a.T.kp;
  const int64_t N = a.N, W = kp + 2;
  const int64_t nh = (int64_t)*a.hot_n;
  for (int64_t j = (int64_t)blockIdx.x * NG + tid / Q; j < nh; j += (int64_t)gridDim.x * NG) {
    const int64_t first = a.hot[j];
    const uint32_t key = a.skeys[first];
    AdaRow<NF> row;
    ada_load_row<Q, NF>(a, key, q, row);
    // pieces of the run: piece m begins at first + m kAdaPiece while that entry carries the key.  Piece 1
    // exists (the run is listed); double m to the first piece beyond the run, then bisect.
    auto in_run = [&](int64_t m) {
      const int64_t pos = first + m * kAdaPiece;
      return pos < N && a.skeys[pos < N ? pos : N - 1] == key;
    };
    int64_t lo = 1, hi = 2;  // in_run(lo), and the answer is the first m > lo that is not
    while (in_run(hi)) {
      lo = hi;
      hi *= 2;
    }
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) / 2;
      if (in_run(mid)) lo = mid;
      else hi = mid;
    }
    const int64_t np = hi;
    double A[C];
#pragma unroll
    for (int c = 0; c < C; ++c) A[c] = 0.0;
    double b = 0.0, gw = 0.0;
#pragma unroll 4
    for (int64_t m = 0; m < np; ++m) {
      const double* pr = a.part + ada_slot(first + m * kAdaPiece, m == 0) * W;
#pragma unroll
      for (int n = 0; n < NF; ++n) {
        const int c = 4 * (q + Q * n);
        if (c < kp) {
          A[4 * n + 0] += pr[1 + c + 0];
          A[4 * n + 1] += pr[1 + c + 1];
          A[4 * n + 2] += pr[1 + c + 2];
          A[4 * n + 3] += pr[1 + c + 3];
        }
      }
      gw += pr[0];
      b += pr[kp + 1];
    }
    ada_apply<Q, NF>(a, key, q, row, A, b, gw);
  }
}

__global__ __launch_bounds__(kBlock) void k_ada_fill(float* __restrict__ G, int64_t rows, int kp, float g0) {
  const int64_t W = kp + 4, n = rows * W;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock)
    G[i] = i % W <= kp ? g0 : 0.f;
}

// the one choice of lane group by kp: 4 lanes up to kp = 16, else 16 lanes of 1, 2 or 4 quads
template <class F>
void with_ada_cfg(int kp, F&& f) {
  if (kp <= 16) f(std::integral_constant<int, 4>{}, std::integral_constant<int, 1>{});
  else if (kp <= 64) f(std::integral_constant<int, 16>{}, std::integral_constant<int, 1>{});
  else if (kp <= 128) f(std::integral_constant<int, 16>{}, std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 16>{}, std::integral_constant<int, 4>{});
}

}  // namespace

}  // namespace fmhip
extern "C" int32_t fm_seam_adagrad_piece(void) { return fmhip::kAdaPiece; }
namespace fmhip {

void AdaWork::ensure(int64_t N, int kp) {
  const size_t n = (size_t)std::max<int64_t>(N, 1);
  const size_t nchunks = (size_t)std::max<int64_t>(pair_scan_chunks(N), 1);
  flag.ensure_slack(sizeof(uint32_t) * n);
  off.ensure_slack(sizeof(int64_t) * (n + 1));
  chunk_tot.ensure_slack(sizeof(int64_t) * nchunks);
  chunk_off.ensure_slack(sizeof(int64_t) * nchunks);
  part.ensure_slack(sizeof(double) * 2 * (n / kAdaPiece + 1) * (size_t)(kp + 2));
  hot.ensure_slack(sizeof(int64_t) * (n / kAdaPiece + 1));
  ucnt.ensure_slack(sizeof(uint32_t) * ((n + kBlock - 1) / kBlock));
  if (!cnt.p) {
    cnt.ensure(64);  // {total, the two alternating list counters}
    FM_HIP_CHECK(hipMemset(cnt.p, 0, 64));
  }
}

void launch_ada_fill(float* G, int64_t rows, int kp, double g0, hipStream_t st) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(k_ada_fill, dim3(grid_for(rows * (kp + 4), kBlock)), dim3(kBlock), 0, st, G, rows, kp, (float)g0);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_adagrad(const TableView& T, float* G, int64_t N, const StepWork& w, AdaWork& aw, const StepParams& p,
                    const uint32_t* skeys, const uint2* sents, int64_t n_loss_blocks, double* stats_out, hipStream_t st) {
  aw.ensure(N, T.kp);
  const StepYl yl = step_yl(w, T.kp);
  AdaArgs a;
  a.T = T;
  a.G = G;
  a.skeys = skeys;
  a.sents = sents;
  a.N = N;
  a.S = w.S.as<float>();
  a.s_stride = s_rec_floats(T.kp);
  a.yl = yl.yl;
  a.yl_stride = yl.stride;
  a.p = p;
  a.off = aw.off.as<int64_t>();
  a.total = aw.cnt.as<int64_t>();
  a.part = aw.part.as<double>();
  a.hot = aw.hot.as<int64_t>();
  unsigned long long* counters = aw.cnt.as<unsigned long long>() + 1;
  a.hot_n = counters + (aw.tick & 1);
  unsigned long long* hot_n_next = counters + ((aw.tick + 1) & 1);
  aw.tick += 1;
  // (a batch without entries still runs the flag pass's one block: it clears the next step's counter)
  const int64_t fblocks = std::max<int64_t>((N + kBlock - 1) / kBlock, 1);
  hipLaunchKernelGGL(k_ada_flag, dim3((unsigned)fblocks), dim3(kBlock), 0, st, skeys, N, aw.flag.as<uint32_t>(),
                     aw.ucnt.as<uint32_t>(), a.hot, a.hot_n, hot_n_next);
  if (N > 0) {
    launch_len_scan(aw.flag.as<uint32_t>(), N, aw.off.as<int64_t>(), aw.chunk_tot.as<int64_t>(), aw.chunk_off.as<int64_t>(),
                    aw.cnt.as<int64_t>(), st);
  }
  with_ada_cfg(T.kp, [&](auto qc, auto nfc) {
    constexpr int Q = decltype(qc)::value, NF = decltype(nfc)::value;
    if (N > 0) {
      // at most N pieces; the groups beyond the device's count leave at once
      hipLaunchKernelGGL((k_ada_piece<Q, NF>), dim3(grid_for(N * Q, kBlock, 256 * 32)), dim3(kBlock), 0, st, a);
    }
    // fewer than N / kAdaPiece runs of several pieces; at least block 0, which closes the step
    hipLaunchKernelGGL((k_ada_fold<Q, NF>), dim3(grid_for((N / kAdaPiece) * Q, kBlock, 1024)), dim3(kBlock), 0, st, a,
                       w.loss_part.as<double2>(), n_loss_blocks, aw.ucnt.as<uint32_t>(), fblocks, stats_out);
  });
  FM_HIP_CHECK(hipGetLastError());
}

}  // namespace fmhip
