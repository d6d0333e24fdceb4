// The wave-per-window update stage of the single-table step for gfx950 (MI355X), defined once and instantiated
// per optimizer rule: FM_OPT_FTRL (fm_ftrl.hip) and FM_OPT_ADAM (fm_adam.hip).  It takes launch_segment_update's
// place in the step (fm_capi.hip step_impl): the same sorted view, S records and {r, yh} pairs in, the table rows
// and their state rows [rows][2 (kp + 4)] = {s0_V[kp], s0_w, a, b, c, s1_V[kp], s1_w, 0, 0, 0} updated, stats[3]
// closed.  Each including file instantiates the kernels for its own rule; nothing here has external linkage.
//
// A rule R supplies
//   R::Hyper                          the host-built hyper-parameters, passed by value in the kernel's arguments
//   R::Row  R::prologue(a, quad)      the row's scalars, once per lane per closing run, from the state quad
//                                     {s0_w, a, b, c} the stage has loaded anyway (FTRL: nothing)
//   float   R::coord(v, g, s0, s1, a, row)   one coordinate: v_cur and the run's fp64 gradient sum in, the two state
//                                     words advanced in place, the new value returned
//   float4  R::state_quad(s0_w, a)    what the quad {s0_w, a, b, c} leaves with (FTRL: {z_w, 0, 0, 0})
// and the stage forms the sums, brings the row current and stores.  The walk never calls the rule: only apply does.
//
// The work is cut by position, as in k_segment_update, not by runs (fm_adagrad.hip cuts by runs):
//   k_ftrl_window  one wave per window of kFtrlWin consecutive sorted entries, four waves per block.
//       Stage.   Each lane loads four entries' key and {sample, x} (coalesced), run heads and ends come from
//                shuffles and ballots, and the window's image {key, flags | sample | x} goes to the wave's LDS,
//                XOR-swizzled so that the groups' reads of one step hit distinct banks.
//       Walk.    Lane groups of Q lanes (kp <= 16: 4 lanes, one float4 column quad each; wider rows 16 lanes and
//                1, 2 or 4 quads) own a stretch of kFtrlWin / (64 / Q) consecutive entries and walk it in entry
//                order into fp64 {A[kp], b, g_w}.  The S quads and {r, yh} of entry e + kFtrlAhead are requested
//                before entry e is consumed: kFtrlAhead entries per group stay in flight throughout, 64 per wave
//                at Q = 4.  The row, header and state row of a run that closes inside the stretch are requested
//                one entry ahead of its last entry.
//       Close.   A run that begins and closes inside one stretch is applied there.  The pieces cut by stretch
//                boundaries meet in LDS (a head piece per group: the run began earlier; a tail piece: it goes on)
//                and are folded in stretch order by the group that holds the run's last entry, which applies the
//                row.  A run that reaches past the window leaves an fp64 partial in global slot 2 w (the window's
//                leading piece, or a run that began earlier and covers the whole window) or 2 w + 1 (its open tail).
//   k_ftrl_fold    one lane group per window w whose tail run is open and begins in w -- decided from the keys at
//                the window edges alone, no list and no atomic -- adds the following windows' slot-2 w' partials
//                in window order until the keys say the run ended, and applies the row.  Block 0 closes the step
//                as k_segment_combine's block 0 does: the loss partials in that kernel's order (a first step
//                reports an SGD step's loss bits) and the distinct ids from the window blocks' head counts.
// Every row and state row is read once and written once, when its run closes; the header's 64-B granule is
// completed (hdr_span) and the state row leaves in whole 16-byte stores.  Every sum runs in a fixed order and there
// are no float atomics: equal batches give equal bits, prepared or sorted inline (the stable sort gives the same
// view).  Unlike the AdaGrad stage, the order of a run's sum depends on where the run lies in the view (which
// stretch and window edges cut it).
#pragma once
#include <algorithm>
#include <type_traits>

#include "fm_device.h"

namespace fmhip {

namespace {

constexpr int kFtrlWin = 256;  // sorted entries per window (one wave)
constexpr int kFtrlAhead = 4;  // entries whose S quads and {r, yh} a lane group keeps in flight
constexpr int kStatLd = 8;     // the closing block's loads in flight per thread (k_segment_combine's)
constexpr int kWavesPerBlock = kBlock / 64;
constexpr uint32_t kFValid = 1u, kFEnd = 2u, kFStart = 4u;
constexpr uint32_t kNoKey = 0xFFFFFFFFu;

template <class R>
struct WinArgs {
  TableView T;
  float* Z;               // [rows][2 (kp + 4)] state rows
  const uint32_t* skeys;  // sorted feature slots
  const uint2* sents;     // their entries {sample, x bits}
  int64_t N;
  const float* S;
  const float2* yl;
  int64_t s_stride, yl_stride;
  StepParams p;
  typename R::Hyper h;
  double inv_m;
  double* part;    // [2 windows][kp + 2] = [g_w | A (kp) | b]
  uint32_t* ucnt;  // [window blocks] run heads
};

// Lane-group geometry: NG groups of Q lanes, a stretch of RL entries each; the image slot of the stretch's
// entry `row` in group g; the LDS regions of a wave.
template <int Q, int NF>
struct FtrlGeom {
  static constexpr int NG = 64 / Q;
  static constexpr int RL = kFtrlWin / NG;
  static constexpr int PIECE = 4 * Q * NF + 2;  // doubles per piece: [g_w | columns | b]
  static __device__ __forceinline__ int at(int row, int g) { return row * NG + (g ^ (row & (NG - 1))); }
  static constexpr int IMG = kFtrlWin * 16;  // {key, flags} (8 B) | sample | x
  // the tail pieces (the last group's goes straight to its global slot) take the image's place once the walk is over
  static constexpr int TAILS = (NG - 1) * PIECE * 8;
  static constexpr int A = IMG > TAILS ? IMG : TAILS;
  static constexpr int HEADS = NG * PIECE * 8;  // written during the walk, as the head pieces close
  static constexpr int BYTES = A + HEADS;
};

// ------------------------------------------------------------------------------- the row update
// One lane's share of a row as it was stored: NF V quads with their two state quads, the header and the state
// row's {s0_w, a, b, c} and {s1_w, 0, 0, 0}.
template <int NF>
struct FtrlRow {
  float4 v[NF], z[NF], n[NF], h, zw, nw;
};
template <class R, int Q, int NF>
__device__ __forceinline__ void ftrl_load_row(const WinArgs<R>& a, uint32_t slot, int q, FtrlRow<NF>& r) {
  const int kp = a.T.kp;
  const float* rec = a.T.v(slot);
  const float* zs = a.Z + (int64_t)slot * (2 * (kp + 4));
  const float* ns = zs + kp + 4;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    const int c = 4 * (q + Q * n);
    r.v[n] = c < kp ? *reinterpret_cast<const float4*>(rec + c) : zero;
    r.z[n] = c < kp ? *reinterpret_cast<const float4*>(zs + c) : zero;
    r.n[n] = c < kp ? *reinterpret_cast<const float4*>(ns + c) : zero;
  }
  r.h = *reinterpret_cast<const float4*>(rec + kp);
  r.zw = *reinterpret_cast<const float4*>(zs + kp);
  r.nw = *reinterpret_cast<const float4*>(ns + kp);
}

// The run's sums applied to its row by the rule.  The row is brought current through the SGD update's helpers
// (pending_l1 and the fp32 soft threshold; an absent row counts as zero) and leaves with next_hdr.
template <class R, int Q, int NF>
__device__ __forceinline__ void ftrl_apply(const WinArgs<R>& a, uint32_t slot, int q, const FtrlRow<NF>& r, const double* A,
                                           double b, double gw) {
  const int kp = a.T.kp;
  const RowHdr h = *reinterpret_cast<const RowHdr*>(&r.h);
  const bool present = h.t >= 0;
  const float acf = present ? pending_l1(h, a.p) : 0.f;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float* rec = a.T.v(slot);
  float* zs = a.Z + (int64_t)slot * (2 * (kp + 4));
  float* ns = zs + kp + 4;
  const typename R::Row rs = R::prologue(a, r.zw);
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    const int c = 4 * (q + Q * n);
    if (c >= kp) continue;
    const QuadGrad qg = quad_grad(present ? r.v[n] : zero, acf, A + 4 * n, b);  // v_cur and g = A - v_cur b
    float4 z = r.z[n], nn = r.n[n], o;
    o.x = R::coord(qg.v.x, qg.g0, z.x, nn.x, a, rs);
    o.y = R::coord(qg.v.y, qg.g1, z.y, nn.y, a, rs);
    o.z = R::coord(qg.v.z, qg.g2, z.z, nn.z, a, rs);
    o.w = R::coord(qg.v.w, qg.g3, z.w, nn.w, a, rs);
    st_row4(rec + c, o);
    st_row4(zs + c, z);
    st_row4(ns + c, nn);
  }
  float zw = r.zw.x, nw = r.nw.x;
  const float w_new = R::coord(present ? shrink1f(h.w, acf) : 0.f, gw, zw, nw, a, rs);
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
  if (q == 0) {
    st_row4(zs + kp, R::state_quad(zw, a));
    st_row4(ns + kp, make_float4(nw, 0.f, 0.f, 0.f));
  }
}

// a lane's share of a piece [g_w | columns | b] to and from LDS or a global slot (row width `cols` columns)
template <int Q, int NF>
__device__ __forceinline__ void piece_put(double* pr, int q, int cols, const double* A, double b, double gw) {
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    const int c = 4 * (q + Q * n);
    if (c < cols) {
      pr[1 + c + 0] = A[4 * n + 0];
      pr[1 + c + 1] = A[4 * n + 1];
      pr[1 + c + 2] = A[4 * n + 2];
      pr[1 + c + 3] = A[4 * n + 3];
    }
  }
  if (q == 0) {
    pr[0] = gw;
    pr[cols + 1] = b;
  }
}
template <int Q, int NF>
__device__ __forceinline__ void piece_add(const double* pr, int q, int cols, double* A, double& b, double& gw) {
#pragma unroll
  for (int n = 0; n < NF; ++n) {
    const int c = 4 * (q + Q * n);
    if (c < cols) {
      A[4 * n + 0] += pr[1 + c + 0];
      A[4 * n + 1] += pr[1 + c + 1];
      A[4 * n + 2] += pr[1 + c + 2];
      A[4 * n + 3] += pr[1 + c + 3];
    }
  }
  gw += pr[0];
  b += pr[cols + 1];
}

// ------------------------------------------------------------------------------- windows
template <class R, int Q, int NF>
__global__ __launch_bounds__(kBlock) void k_ftrl_window(WinArgs<R> a) {
  using Geo = FtrlGeom<Q, NF>;
  constexpr int NG = Geo::NG, RL = Geo::RL, PIECE = Geo::PIECE, NP = kFtrlWin / 64, C = 4 * NF;
  constexpr int D = kFtrlAhead;
  static_assert(RL % D == 0 && D % 2 == 0, "the walk is unrolled by D, the row buffers alternate");
  constexpr int KPW = 4 * Q * NF;  // the LDS pieces' column count (the widest kp served)
  __shared__ __align__(16) unsigned char smem_all[kWavesPerBlock][Geo::BYTES];
  __shared__ int pflag_all[kWavesPerBlock][2 * NG];
  __shared__ uint32_t wcnt[kWavesPerBlock];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned char* smem = smem_all[wave];
  uint2* img_k = reinterpret_cast<uint2*>(smem);                      // {slot, flags}
  int* img_s = reinterpret_cast<int*>(smem + kFtrlWin * 8);           // sample
  float* img_x = reinterpret_cast<float*>(smem + kFtrlWin * 12);      // x
  double* tails = reinterpret_cast<double*>(smem);                    // [NG - 1][PIECE], after the walk
  double* heads = reinterpret_cast<double*>(smem + Geo::A);           // [NG][PIECE]
  int* pflag = pflag_all[wave];
  const int kp = a.T.kp;
  const int64_t N = a.N;
  const int64_t wid = (int64_t)blockIdx.x * kWavesPerBlock + wave;
  const int64_t base = wid * kFtrlWin;
  uint32_t ucount = 0;

  if (base < N) {  // wave-uniform
    // ---------------- stage: one lane per entry, four entries per lane
    uint32_t key[NP];
    uint2 en[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int64_t p = base + i * 64 + lane;
      const bool v = p < N;
      key[i] = v ? a.skeys[p] : kNoKey;
      en[i] = v ? a.sents[p] : make_uint2(0u, 0u);
    }
    const uint32_t before = base > 0 ? a.skeys[base - 1] : kNoKey;
    const uint32_t after = base + kFtrlWin < N ? a.skeys[base + kFtrlWin] : kNoKey;
    // the key of the run that began before the window and leads it (kNoKey: the window begins with a run's head)
    const uint32_t first_key = __shfl(key[0], 0);
    const uint32_t lead_key = first_key == before ? first_key : kNoKey;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const uint32_t up = __shfl_up(key[i], 1);
      const uint32_t dn = __shfl_down(key[i], 1);
      const uint32_t pl = i > 0 ? __shfl(key[i > 0 ? i - 1 : 0], 63) : before;
      const uint32_t nf = i + 1 < NP ? __shfl(key[i + 1 < NP ? i + 1 : i], 0) : after;
      const uint32_t prev = lane == 0 ? pl : up;
      const uint32_t next = lane == 63 ? nf : dn;
      const bool valid = key[i] != kNoKey;
      const bool st = valid && key[i] != prev;
      const bool end = valid && key[i] != next;
      ucount += (uint32_t)__popcll(__ballot(st));
      const int e = i * 64 + lane;
      const int l = Geo::at(e % RL, e / RL);
      img_k[l] = make_uint2(key[i], (valid ? kFValid : 0u) | (end ? kFEnd : 0u) | (st ? kFStart : 0u));
      img_s[l] = (int)en[i].x;
      img_x[l] = __uint_as_float(en[i].y);
    }
    wave_lds_sync();

    // ---------------- walk: group g, lane q of the group
    const int g = lane / Q, q = lane % Q;
    float4 Sb[D][NF];
    float2 Yb[D];  // the samples' {r, yh}
    auto request = [&](int b, float4 (&Sq)[NF], float2& y) {
      const int l = Geo::at(b, g);
      const bool valid = (img_k[l].y & kFValid) != 0;
      const int64_t s = (int64_t)img_s[l];
#pragma unroll
      for (int n = 0; n < NF; ++n) {
        const int c = 4 * (q + Q * n);
        Sq[n] = (valid && c < kp) ? *reinterpret_cast<const float4*>(a.S + s * a.s_stride + c) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
      y = valid ? a.yl[s * a.yl_stride] : make_float2(0.f, 0.f);
    };
#pragma unroll
    for (int u = 0; u < D; ++u) request(u, Sb[u], Yb[u]);
    // the rows of the runs that close inside the stretch, requested one entry ahead: two buffers in turn
    FtrlRow<NF> rows[2];
    {
      const uint2 k0 = img_k[Geo::at(0, g)];
      if ((k0.y & (kFValid | kFStart | kFEnd)) == (kFValid | kFStart | kFEnd)) ftrl_load_row<R, Q, NF>(a, k0.x, q, rows[0]);
    }
    double acc[C];
#pragma unroll
    for (int j = 0; j < C; ++j) acc[j] = 0.0;
    double accb = 0.0, accw = 0.0;
    int hst = 0;  // the group's head piece: 0 none, 1 open through the stretch's end, 2 closed
    uint32_t head_key = kNoKey;
    bool started = false, open = false;
#pragma unroll 1
    for (int b0 = 0; b0 < RL; b0 += D) {
#pragma unroll
      for (int u = 0; u < D; ++u) {
        const int b = b0 + u;
        const int l = Geo::at(b, g);
        const uint2 kf = img_k[l];
        const double xd = (double)img_x[l];
        float4 Sc[NF];
#pragma unroll
        for (int n = 0; n < NF; ++n) Sc[n] = Sb[u][n];
        const float2 yc = Yb[u];
        const bool st_b = started || (kf.y & kFStart);
        if (b + 1 < RL) {
          const uint2 kn = img_k[Geo::at(b + 1, g)];
          const bool st_n = ((kf.y & kFEnd) ? false : st_b) || (kn.y & kFStart);
          if ((kn.y & kFValid) && (kn.y & kFEnd) && st_n) ftrl_load_row<R, Q, NF>(a, kn.x, q, rows[(u + 1) & 1]);
        }
        if (b + D < RL) request(b + D, Sb[u], Yb[u]);
        if (kf.y & kFValid) {
          // t = x r, x^2 r and g_w = (x - 1) yh + r, as the SGD update forms them
          const double rj = (double)yc.x, yh = (double)yc.y;
          const double t = xd * rj;
          started = st_b;
          open = true;
#pragma unroll
          for (int n = 0; n < NF; ++n) {
            acc[4 * n + 0] = fma((double)Sc[n].x, t, acc[4 * n + 0]);
            acc[4 * n + 1] = fma((double)Sc[n].y, t, acc[4 * n + 1]);
            acc[4 * n + 2] = fma((double)Sc[n].z, t, acc[4 * n + 2]);
            acc[4 * n + 3] = fma((double)Sc[n].w, t, acc[4 * n + 3]);
          }
          accb += (xd * xd) * rj;
          accw += (xd - 1.0) * yh + rj;
          if (kf.y & kFEnd) {
            if (started) {
              ftrl_apply<R, Q, NF>(a, kf.x, q, rows[u & 1], acc, accb, accw);
            } else {  // the head piece closes
              piece_put<Q, NF>(heads + g * PIECE, q, KPW, acc, accb, accw);
              hst = 2;
              head_key = kf.x;
            }
#pragma unroll
            for (int j = 0; j < C; ++j) acc[j] = 0.0;
            accb = 0.0;
            accw = 0.0;
            started = false;
            open = false;
          }
        }
      }
    }
    const bool tail = open && started;  // the open piece began in this stretch
    if (open && !started) {             // the head piece runs through the stretch's end
      piece_put<Q, NF>(heads + g * PIECE, q, KPW, acc, accb, accw);
      hst = 1;
    }
    // a closed head piece whose run began inside the window is applied below, by this group: its row now
    const bool head_row = hst == 2 && head_key != lead_key;
    FtrlRow<NF> hrow;
    if (head_row) ftrl_load_row<R, Q, NF>(a, head_key, q, hrow);

    // ---------------- close: the pieces cut by stretch boundaries (the image is dead now)
    wave_lds_sync();
    if (tail && g < NG - 1) piece_put<Q, NF>(tails + g * PIECE, q, KPW, acc, accb, accw);
    if (q == 0) {
      pflag[2 * g] = hst;
      pflag[2 * g + 1] = tail ? 1 : 0;
    }
    wave_lds_sync();
    const int W = kp + 2;
    if (hst == 2 || (g == NG - 1 && hst == 1)) {
      // the group holding the run's last entry inside the window: back over the stretches the run covers whole
      // to the one it began in (g0; -1: before the window), then the pieces in stretch order
      int g0 = g - 1;
      while (g0 >= 0 && pflag[2 * g0] == 1) --g0;
      double fa[C], fb = 0.0, fw = 0.0;
#pragma unroll
      for (int j = 0; j < C; ++j) fa[j] = 0.0;
      if (g0 >= 0) piece_add<Q, NF>(tails + g0 * PIECE, q, KPW, fa, fb, fw);  // 0 + x: the tail piece itself
      for (int g2 = g0 + 1; g2 <= g; ++g2) piece_add<Q, NF>(heads + g2 * PIECE, q, KPW, fa, fb, fw);
      if (g0 >= 0 && hst == 2) ftrl_apply<R, Q, NF>(a, head_key, q, hrow, fa, fb, fw);
      else piece_put<Q, NF>(a.part + (wid * 2 + (g0 >= 0 ? 1 : 0)) * (int64_t)W, q, kp, fa, fb, fw);
    }
    // a run that begins in the last stretch and is open at the window's end
    if (tail && g == NG - 1) piece_put<Q, NF>(a.part + (wid * 2 + 1) * (int64_t)W, q, kp, acc, accb, accw);
  }
  if (lane == 0) wcnt[wave] = ucount;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) t += wcnt[w];
    a.ucnt[blockIdx.x] = t;
  }
}

// ------------------------------------------------------------------------------- fold and close
template <class R, int Q, int NF>
__global__ __launch_bounds__(kBlock) void k_ftrl_fold(WinArgs<R> a, const double2* __restrict__ loss_part, int64_t n_loss_blocks,
                                                      int64_t n_ucnt, double* __restrict__ stats_out) {
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
    for (int64_t i = tid; i < n_ucnt; i += kBlock) u += (double)a.ucnt[i];  // whole numbers: exact in any order
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
  const int64_t nwin = (N + kFtrlWin - 1) / kFtrlWin;
  // window w owns a run when its last entry's run goes on into w + 1 and began in w (the last window owns none)
  for (int64_t w = (int64_t)blockIdx.x * NG + tid / Q; w + 1 < nwin; w += (int64_t)gridDim.x * NG) {
    const int64_t first = w * kFtrlWin, last = first + kFtrlWin - 1;
    const uint32_t key = a.skeys[last];
    if (a.skeys[last + 1] != key) continue;
    if (a.skeys[first] == key && first > 0 && a.skeys[first - 1] == key) continue;  // began before w
    FtrlRow<NF> row;
    ftrl_load_row<R, Q, NF>(a, key, q, row);
    double A[C];
#pragma unroll
    for (int c = 0; c < C; ++c) A[c] = 0.0;
    double b = 0.0, gw = 0.0;
    piece_add<Q, NF>(a.part + (2 * w + 1) * W, q, kp, A, b, gw);  // 0 + x: the open tail itself
    for (int64_t w2 = w + 1;; ++w2) {
      // the leading (or whole-window) piece of w2, and whether the run goes on behind w2
      const int64_t nx = (w2 + 1) * kFtrlWin;
      const bool more = nx < N && a.skeys[nx < N ? nx : N - 1] == key;
      piece_add<Q, NF>(a.part + 2 * w2 * W, q, kp, A, b, gw);
      if (!more) break;
    }
    ftrl_apply<R, Q, NF>(a, key, q, row, A, b, gw);
  }
}

// the one choice of lane group by kp: 4 lanes up to kp = 16, else 16 lanes of 1, 2 or 4 quads
template <class F>
void with_ftrl_cfg(int kp, F&& f) {
  if (kp <= 16) f(std::integral_constant<int, 4>{}, std::integral_constant<int, 1>{});
  else if (kp <= 64) f(std::integral_constant<int, 16>{}, std::integral_constant<int, 1>{});
  else if (kp <= 128) f(std::integral_constant<int, 16>{}, std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 16>{}, std::integral_constant<int, 4>{});
}

// The stage's two launches for rule R with its hyper-parameters h (everything else is the step's).
template <class R>
void launch_window_stage(const TableView& T, float* Z, int64_t N, const StepWork& w, FtrlWork& fw, const StepParams& p,
                         const typename R::Hyper& h, const uint32_t* skeys, const uint2* sents, int64_t n_loss_blocks,
                         double* stats_out, hipStream_t st) {
  fw.ensure(N, T.kp);
  const StepYl yl = step_yl(w, T.kp);
  WinArgs<R> a;
  a.T = T;
  a.Z = Z;
  a.skeys = skeys;
  a.sents = sents;
  a.N = N;
  a.S = w.S.as<float>();
  a.s_stride = s_rec_floats(T.kp);
  a.yl = yl.yl;
  a.yl_stride = yl.stride;
  a.p = p;
  a.h = h;
  a.inv_m = 1.0 / p.m;
  a.part = fw.part.as<double>();
  a.ucnt = fw.ucnt.as<uint32_t>();
  const int64_t nwin = (N + kFtrlWin - 1) / kFtrlWin;
  const int64_t wblocks = (nwin + kWavesPerBlock - 1) / kWavesPerBlock;
  with_ftrl_cfg(T.kp, [&](auto qc, auto nfc) {
    constexpr int Q = decltype(qc)::value, NF = decltype(nfc)::value;
    if (wblocks > 0) hipLaunchKernelGGL((k_ftrl_window<R, Q, NF>), dim3((unsigned)wblocks), dim3(kBlock), 0, st, a);
    // one lane group per window; at least block 0, which closes the step
    hipLaunchKernelGGL((k_ftrl_fold<R, Q, NF>), dim3(grid_for(nwin * Q, kBlock, 1024)), dim3(kBlock), 0, st, a,
                       w.loss_part.as<double2>(), n_loss_blocks, wblocks, stats_out);
  });
  FM_HIP_CHECK(hipGetLastError());
}

}  // namespace

}  // namespace fmhip
