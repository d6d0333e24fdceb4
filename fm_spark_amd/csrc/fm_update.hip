// The update side of the FM SGD step for gfx950 (MI355X): the segmented update over the sorted
// entries (k_segment_update), the combine of the runs that cross its waves (k_segment_combine), the
// replicated mode's apply (k_repl_apply, k_sum_counts) and the fused step's singleton split
// (k_split_*).  The step as a whole, and the row arithmetic these kernels share with the fused
// forward: fm_device.h.
#include <algorithm>
#include <cstdlib>

#include "fm_device.h"

namespace fmhip {

namespace {

constexpr int kWaveEnt = 256;  // sorted entries per update wave
constexpr int kUpdD = 2;   // entries whose rows a lane group loads per step
// (two entries ahead at k = 5..8 or 13..16 measured slower at c2 / c5 / c3: profiles/r04_o)
constexpr int kUpdD4 = 1;  // k = 13..16 (4 lanes per entry, paired row stores): one entry ahead keeps the
                           // kernel within the 5-wave register budget
constexpr int kUpdD2 = 1;  // k = 5..8 (2 lanes per entry, paired row stores)

// -------------------------------------------------------------- segmented update
struct SegArgs {
  TableView T;
  const uint32_t* skeys;  // sorted feature slots
  const uint2* sents;     // their entries {sample, x bits}, same order
  int64_t N;
  const float* S;    // per-sample rows of s_stride floats (vfxiSum first)
  const float2* yl;  // {r = yhat - y, yhat} of sample s at yl[s * yl_stride]
  int64_t s_stride;
  int64_t yl_stride;
  double* part;      // [nranges][2][kp + 2] = [sum g_w | sum S*x*r (kp) | sum x*x*r]
  int64_t nranges;   // ranges of L sorted entries (one update wave each)
  int64_t L;         // entries per range (kWaveEnt)
  StepParams p;
  uint32_t* ucnt;  // [update blocks]
  float* emit;     // replicated mode: per-slot gradient sums [rows][kp + 4] instead of the update
  // non-null: the entry count is n_dev[0] <= N (a prepared batch's multi runs, counted on the
  // device by k_split_*), and n_dev[1] distinct singleton rows were updated by the forward
  const int64_t* n_dev;
};

constexpr uint32_t kFValid = 1u, kFEnd = 2u, kFStart = 4u;


// Lane-group geometry: Q lanes per entry, NF float4 column quads per lane (columns
// 4 (q + Q n) .. + 3), NG = 64 / Q groups per wave, RL = 256 / NG entries per group.
template <int Q, int NF>
struct UpdGeom {
  static constexpr int NG = 64 / Q;
  static constexpr int RL = kWaveEnt / NG;
  static constexpr int KP = 4 * Q * NF;   // widest kp served
  static constexpr int PIECE = KP + 2;    // doubles per piece: [g_w | columns | b]
  static constexpr int IMG_N = RL * NG;   // image slots: RL rows of NG, column g XOR-swizzled by the
                                          // row against bank conflicts (no pad column: at k = 32 the
                                          // pad cost the fourth block per CU)
  static __device__ __forceinline__ int at(int row, int g) { return row * NG + (g ^ (row & (NG - 1))); }
  // image entry: {slot, flags} | sample | x (16 B)
  static constexpr int IMG = IMG_N * 16;
  // the groups' head pieces go to their own region after the image as they close (one slot per
  // group) instead of living in registers until phase 3
  static constexpr int HEADS = NG * PIECE * 8;
  static constexpr int BYTES = IMG + HEADS;
  // the configurations whose rows leave in paired stores at kp = 4Q (k_segment_update, "Paired row stores")
  static constexpr bool PAIR = (Q == 2 || Q == 4) && NF == 1;
};

// The one choice of k_segment_update<Q, NF, D> by kp: f is called with the UpdCfg of the
// instantiation that serves kp (the launch and update_geometry both go through here).
template <int Q_, int NF_, int D_>
struct UpdCfg {
  static constexpr int Q = Q_, NF = NF_, D = D_;
};
template <class F>
void with_update_cfg(int kp, F&& f) {
  const int nq = kp / 4;  // column quads
  if (nq <= 1) f(UpdCfg<1, 1, kUpdD>{});
  else if (nq <= 2) f(UpdCfg<2, 1, kUpdD2>{});
  else if (nq <= 4) f(UpdCfg<4, 1, kUpdD4>{});
  else if (nq <= 8) f(UpdCfg<8, 1, kUpdD>{});
  else if (nq <= 16) f(UpdCfg<16, 1, kUpdD>{});
  else if (nq <= 32) f(UpdCfg<16, 2, 2>{});
  else f(UpdCfg<16, 4, 1>{});
}

// The interaction gradient of one entry (Model.scala:201-204, SGD.scala:146) is
//   g_V[f] = (S[s][f] * x - (v[f] * x) * x) * r,   r = yhat - y,
// so a feature's run sums to   A[f] - v[f] * b,   A[f] = sum_e S[s_e][f] * (x_e r_e),
// b = sum_e x_e^2 r_e: neither sum needs the row, which is read once per run, with its header,
// when the run closes.  g_w = x * yhat - y per entry (SGD.scala:145).
//
// One wave per 256 sorted entries.
//  Phase 1, one lane per entry: run structure (ballots), staged in the wave's LDS image with the
//    entry's sample and x (16 B per entry, step-major so that a step's entries are contiguous).
//  Phase 2, NG lane groups of Q lanes (float4 column quads per lane): group g walks its RL
//    consecutive entries in order, accumulating A, b and g_w in fp64 from the S rows and {r, yhat}
//    of D entries loaded ahead (one record per sample in the single-table step, FM_S_REC; with
//    the V row + header of those that close a run): t = x r, x^2 r and x yhat - y per entry.  A run that
//    begins and closes inside the group's entries is applied in place (update + L1,
//    SGD.scala:150-181, or its gradient emitted in replicated mode).
//  Phase 3: the pieces cut by group boundaries meet in LDS: the group holding a run's start
//    extends its open piece through the following groups' head pieces and applies the run when
//    it closes inside the wave; the wave's first piece (run begun in an earlier wave) and a run
//    still open at the wave's end leave fp64 partials (slot 0 / slot 1), summed in wave order by
//    k_segment_combine.  Every sum runs in a fixed order: the step is bitwise reproducible.
// k <= 64 (NF = 1): waves per SIMD the register allocation must allow (4 blocks/CU); without it the
// compiler took 130 VGPRs at k = 16 (3 waves/SIMD): update -8.6 %, step -1.7 % (A/B 3 x 40 steps)
// (round 3: 5 waves, 96 VGPRs with 32 B/lane spilled at k = 16, measured 0.981-0.984 against
// 0.986-0.990 ms at c3 and 0.192-0.193 against 0.194-0.195 at c5: within the noise, not taken)
constexpr int kUpdMinW = 4;
template <int Q, int NF, int D0>
__global__ __launch_bounds__(kBlock, NF == 1 ? kUpdMinW : 1) void k_segment_update(SegArgs a) {
  using Geo = UpdGeom<Q, NF>;
  constexpr int NG = Geo::NG, RL = Geo::RL, PIECE = Geo::PIECE, NP = kWaveEnt / 64, C = 4 * NF;
  constexpr int D = D0 < RL ? D0 : RL;  // entries loaded ahead (divides RL)
  __shared__ __align__(16) unsigned char smem_all[kBlock / 64][Geo::BYTES];
  __shared__ int pflag_all[kBlock / 64][2 * NG];
  __shared__ uint32_t wcnt[kBlock / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  unsigned char* smem = smem_all[wave];
  constexpr int IN = Geo::IMG_N;
  uint2* img_k = reinterpret_cast<uint2*>(smem);            // {slot, flags}
  int* img_s = reinterpret_cast<int*>(smem + IN * 8);       // sample
  float* img_x = reinterpret_cast<float*>(smem + IN * 12);  // x
  int* pflag = pflag_all[wave];
  const TableView& T = a.T;
  const int kp = T.kp;
  const uint32_t kNone = 0xFFFFFFFFu;
  auto li = [](int e) { return Geo::at(e % RL, e / RL); };
  const int64_t N = a.n_dev ? a.n_dev[0] : a.N;
  // logical blocks of 4 waves x 256 entries (one per block of the grid; blocks beyond a device count exit)
  const int64_t nlblk = (N + (int64_t)kWaveEnt * (kBlock / 64) - 1) / ((int64_t)kWaveEnt * (kBlock / 64));
  for (int64_t lblk = blockIdx.x; lblk < nlblk; lblk += gridDim.x) {
  const int64_t wid = lblk * (kBlock / 64) + wave;
  const int64_t base = wid * kWaveEnt;
  uint32_t ucount = 0;

  if (base < N) {  // wave-uniform
    // ---------------- phase 1: one lane per entry
    uint32_t key[NP];
    uint2 en[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int64_t p = base + i * 64 + lane;
      const bool v = p < N;
      key[i] = v ? a.skeys[p] : kNone;
      en[i] = v ? a.sents[p] : make_uint2(0u, 0u);
    }
    const uint32_t before = base > 0 ? a.skeys[base - 1] : kNone;
    const uint32_t after = base + kWaveEnt < N ? a.skeys[base + kWaveEnt] : kNone;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const uint32_t up = __shfl_up(key[i], 1);
      const uint32_t dn = __shfl_down(key[i], 1);
      const uint32_t pl = i > 0 ? __shfl(key[i > 0 ? i - 1 : 0], 63) : before;
      const uint32_t nf = i + 1 < NP ? __shfl(key[i + 1 < NP ? i + 1 : i], 0) : after;
      const uint32_t prev = lane == 0 ? pl : up;
      const uint32_t next = lane == 63 ? nf : dn;
      const bool valid = key[i] != kNone;
      const bool st = valid && key[i] != prev;
      const bool end = valid && key[i] != next;
      ucount += (uint32_t)__popcll(__ballot(st));
      const int l = li(i * 64 + lane);
      img_k[l] = make_uint2(key[i], (valid ? kFValid : 0u) | (end ? kFEnd : 0u) | (st ? kFStart : 0u));
      img_s[l] = (int)en[i].x;
      img_x[l] = __uint_as_float(en[i].y);
    }
    wave_lds_sync();

    // ---------------- phase 2: group g, lane q of the group
    const int g = lane / Q, q = lane % Q;
    // D entries loaded ahead (one buffer: the next step's loads are issued after a step is consumed)
    float4 Sp0[D][NF], Vp0[D][NF], Hp0[D];
    float2 Yp0[D];  // the samples' {r, yhat}
    auto prefetch = [&](int b0, float4 (&Sp)[D][NF], float4 (&Vp)[D][NF], float4 (&Hp)[D], float2 (&Yp)[D]) {
#pragma unroll
      for (int u = 0; u < D; ++u) {
        const int l = Geo::at(b0 + u, g);  // li(g * RL + b0 + u)
        const uint2 kf = img_k[l];
        const int s = img_s[l];
        const bool valid = (kf.y & kFValid) != 0, end = (kf.y & kFEnd) != 0;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
          const int c = 4 * (q + Q * n);
          const bool cv = valid && c < kp;
          Sp[u][n] = cv ? *reinterpret_cast<const float4*>(a.S + (int64_t)s * a.s_stride + c)
                        : make_float4(0.f, 0.f, 0.f, 0.f);
          Vp[u][n] = (valid && c < kp && end) ? *reinterpret_cast<const float4*>(T.v(kf.x) + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        Hp[u] = (valid && end) ? *reinterpret_cast<const float4*>(T.hdr(kf.x)) : make_float4(0.f, __int_as_float(-1), 0.f, 0.f);
        Yp[u] = valid ? a.yl[(int64_t)s * a.yl_stride] : make_float2(0.f, 0.f);
      }
    };
    prefetch(0, Sp0, Vp0, Hp0, Yp0);

    // Paired row stores (kp = 4Q, Q = 2 or 4: records of V (16Q B) + a header granule of the same
    // size, i.e. k = 5..8 in 64 B and k = 13..16 in 128 B): the new row of a run closed in phase 2
    // is kept in registers and written at the end of the entry step by 2Q lanes, the group's Q (V)
    // and its neighbour group's Q (header + zero pad), so every row leaves in ONE store
    // instruction covering its whole record instead of two half-record ones.
    constexpr bool kPairCfg = Geo::PAIR;
    const bool paired = kPairCfg && kp == 4 * Q && !a.emit;  // wave-uniform
    float4 pend_v = make_float4(0.f, 0.f, 0.f, 0.f);
    float pend_w = 0.f;             // the row's new w (its header is {w, epoch + 1, cum_next})
    uint32_t pend_slot = kNone;     // kNone: nothing pending
    const int span = hdr_span(kp);  // the header and the zero pad of its 64-B granule

    // apply (or emit) a closed run: the row brought current (absent rows are all zero with
    // cum = 0, so they need no case of their own), then SGD.scala:150-181
    auto close_run = [&](uint32_t slot, const float4 (&vq)[NF], float4 hq, const double (&A)[C], double b, double gw,
                         bool defer) {
      const RowHdr h = *reinterpret_cast<const RowHdr*>(&hq);
      const float acf = pending_l1(h, a.p);
      float* rec = T.v(slot);
      if (kPairCfg && defer) {  // this lane's V quad and (lane q = 0) the header, written by flush_pair
        pend_v = upd_quad(vq[0], acf, A, b, a.p);
        pend_w = upd_w_row(h, acf, gw, a.p);
        pend_slot = slot;
        return;
      }
#pragma unroll
      for (int n = 0; n < NF; ++n) {
        const int c = 4 * (q + Q * n);
        if (c >= kp) continue;
        const QuadGrad qg = quad_grad(vq[n], acf, A + 4 * n, b);
        if (a.emit) {
          *reinterpret_cast<float4*>(a.emit + (int64_t)slot * (kp + 4) + c) =
              make_float4((float)qg.g0, (float)qg.g1, (float)qg.g2, (float)qg.g3);
        } else {
          st_row4(rec + c, quad_apply(qg, a.p));
        }
      }
      if (a.emit) {
        if (q == 0) *reinterpret_cast<float2*>(a.emit + (int64_t)slot * (kp + 4) + kp) = make_float2((float)gw, 1.f);
        return;
      }
      // the header and the zero pad of its 64-B granule: the granule is written whole
      for (int i = 4 * q; i < span; i += 4 * Q) {
        float4 hv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i == 0) {
          const RowHdr o = next_hdr(upd_w_row(h, acf, gw, a.p), a.p);
          hv = *reinterpret_cast<const float4*>(&o);
        }
        st_row4(rec + kp + i, hv);
      }
    };
    // the rows closed in this entry step (all lanes, converged): even groups' rows, then odd
    // groups'; the partner group (lane ^ Q) writes the header granule of the row
    auto flush_pair = [&]() {
      // ds_swizzle bit mode within 32 lanes: and 0x1F, or 0, xor Q -> lane ^ Q
      auto swz = [](uint32_t v) { return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, 0x1F | (Q << 10)); };
      const uint32_t p_slot = swz(pend_slot);
      const float p_w = __uint_as_float(swz(__float_as_uint(pend_w)));
      float4 p_h = make_float4(0.f, 0.f, 0.f, 0.f);  // the partner row's header granule: lane q = 0 the header
      if (q == 0) {
        const RowHdr o = next_hdr(p_w, a.p);
        p_h = *reinterpret_cast<const float4*>(&o);
      }
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
        const bool writer = (g & 1) == pass;
        const uint32_t slot = writer ? pend_slot : p_slot;
        // the header granule is 4 + pad floats: 4Q of them at kp = 4Q <= 16
        if (slot != kNone && (writer || 4 * q < span)) st_row4(T.v(slot) + (writer ? 4 * q : kp + 4 * q), writer ? pend_v : p_h);
      }
      pend_slot = kNone;
    };

    double* heads = reinterpret_cast<double*>(smem + Geo::IMG);  // [NG][PIECE]
    auto put_head = [&](const double (&A)[C], double b, double gw) {
      double* ph = heads + g * PIECE;
#pragma unroll
      for (int n = 0; n < NF; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) ph[1 + 4 * (q + Q * n) + j] = A[4 * n + j];
      if (q == 0) {
        ph[0] = gw;
        ph[PIECE - 1] = b;
      }
    };
    double acc[C];
#pragma unroll
    for (int j = 0; j < C; ++j) acc[j] = 0.0;
    double accb = 0.0, accw = 0.0;
    int hst = 0;  // the group's head piece: 0 none, 1 open through the group's end, 2 closed
    bool started = false, open = false;
    uint32_t lastkey = kNone;
    auto consume = [&](int b0, const float4 (&Sp)[D][NF], const float4 (&Vp)[D][NF], const float4 (&Hp)[D],
                       const float2 (&Yp)[D]) {
#pragma unroll
      for (int u = 0; u < D; ++u) {
        const int l = Geo::at(b0 + u, g);
        const uint2 kf = img_k[l];
        if (kf.y & kFValid) {
        // t = x r, x^2 r and g_w = deltaWi * pred - label = x yhat - (yhat - r) (SGD.scala:145)
        const double xd = (double)img_x[l], rj = (double)Yp[u].x, yh = (double)Yp[u].y;
        const double t = xd * rj;
        const double2 tb = make_double2(t, (xd * xd) * rj);
        const double gwe = (xd - 1.0) * yh + rj;
        if (kf.y & kFStart) started = true;
        open = true;
        lastkey = kf.x;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
          acc[4 * n + 0] = fma((double)Sp[u][n].x, t, acc[4 * n + 0]);
          acc[4 * n + 1] = fma((double)Sp[u][n].y, t, acc[4 * n + 1]);
          acc[4 * n + 2] = fma((double)Sp[u][n].z, t, acc[4 * n + 2]);
          acc[4 * n + 3] = fma((double)Sp[u][n].w, t, acc[4 * n + 3]);
        }
        accb += tb.y;
        accw += gwe;
        if (kf.y & kFEnd) {
          if (started) {
            close_run(kf.x, Vp[u], Hp[u], acc, accb, accw, paired);
          } else {  // the head piece closes
            put_head(acc, accb, accw);
            hst = 2;
          }
#pragma unroll
          for (int j = 0; j < C; ++j) acc[j] = 0.0;
          accb = 0.0;
          accw = 0.0;
          started = false;
          open = false;
        }
        }
        // converged: every lane of the wave (with one entry per step, after the next step's
        // loads: see the loop below)
        if (kPairCfg && paired && D > 1) flush_pair();
      }
    };
#pragma unroll 1
    for (int b0 = D; b0 <= RL; b0 += D) {  // the first step's loads are in flight already
      consume(b0 - D, Sp0, Vp0, Hp0, Yp0);
      if (b0 < RL) prefetch(b0, Sp0, Vp0, Hp0, Yp0);
      // the closed rows' stores after the next step's loads: issued before them, the loads had to
      // wait for the stores to complete (their destination registers held the stores' data)
      if (kPairCfg && paired && D == 1) flush_pair();
    }
    const bool tail = open && started;  // the open piece began in this group
    if (open && !started) {             // the head piece runs through the group's end
      put_head(acc, accb, accw);
      hst = 1;
    }

    // ---------------- phase 3: pieces cut by group boundaries (the image is dead now)
    wave_lds_sync();
    double* pc = heads;  // head piece of group g at pc + g * PIECE, written in phase 2
    if (q == 0) pflag[2 * g] = hst;
    wave_lds_sync();
    // extend a piece through the head pieces of groups g2 = from, from + 1, ...; true when it closes
    auto extend = [&](double (&A)[C], double& b, double& gw, int from) -> bool {
      for (int g2 = from; g2 < NG; ++g2) {
        const int f2 = pflag[2 * g2];
        if (f2 == 0) return false;  // unreachable: an open piece always continues into a head piece
        const double* ph = pc + g2 * PIECE;
#pragma unroll
        for (int n = 0; n < NF; ++n)
#pragma unroll
          for (int j = 0; j < 4; ++j) A[4 * n + j] += ph[1 + 4 * (q + Q * n) + j];
        gw += ph[0];
        b += ph[PIECE - 1];
        if (f2 == 2) return true;
      }
      return false;
    };
    const int W = kp + 2;
    auto write_part = [&](int slot, const double (&A)[C], double b, double gw) {
      double* pr = a.part + (wid * 2 + slot) * (int64_t)W;
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
    };
    if (g == 0 && hst) {  // the wave's first piece: its run began in an earlier wave
      double hacc[C], hb = pc[PIECE - 1], hw = pc[0];
#pragma unroll
      for (int n = 0; n < NF; ++n)
#pragma unroll
        for (int j = 0; j < 4; ++j) hacc[4 * n + j] = pc[1 + 4 * (q + Q * n) + j];
      if (hst == 1) extend(hacc, hb, hw, 1);
      write_part(0, hacc, hb, hw);
    }
    if (tail) {
      if (extend(acc, accb, accw, g + 1)) {
        float4 vq[NF];
#pragma unroll
        for (int n = 0; n < NF; ++n) {
          const int c = 4 * (q + Q * n);
          vq[n] = c < kp ? *reinterpret_cast<const float4*>(T.v(lastkey) + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float4 hq = *reinterpret_cast<const float4*>(T.hdr(lastkey));
        close_run(lastkey, vq, hq, acc, accb, accw, false);
      } else {
        write_part(1, acc, accb, accw);  // still open at the wave's end
      }
    }
  }
  if (lane == 0) wcnt[wave] = ucount;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) t += wcnt[w];
    a.ucnt[lblk] = t;
  }
  __syncthreads();  // the image and the counts are reused by the next logical block
  }
}

// Runs that cross range boundaries: the range holding the run's first entry owns it and sums
// the following ranges' head partials in range order (a lane alone when the run ends in the
// next range, one wave per run with lanes over the factor columns otherwise), then applies the
// same update as k_segment_update:  g_V[f] = sum S*x*r [f] - v[f] * sum x*x*r.  Block 0 also
// closes the step with fixed-order reductions.
// The row of `key` brought current, then columns [c_lo, c_hi) step c_step of the run's update
// (sums[j] = sum S*x*r of column c_lo + j * c_step), then its header.
struct RowCur {
  bool present;
  double ac;
  float w;
};
__device__ __forceinline__ RowCur row_current(const SegArgs& a, uint32_t key) {
  const RowHdr h = *a.T.hdr(key);
  RowCur r;
  r.present = h.t >= 0;
  r.ac = r.present ? a.p.cumE - h.cum : 0.0;
  r.w = r.present ? h.w : 0.f;
  if (r.ac > 0.0) r.w = shrink_f(r.w, r.ac);
  return r;
}
// column c of the run's update from the row's stored value vraw (read whatever the row's presence)
__device__ __forceinline__ void close_col(const SegArgs& a, uint32_t key, const RowCur& rc, int c, float vraw, double b,
                                          double sum) {
  float v = rc.present ? vraw : 0.f;
  if (rc.ac > 0.0) v = shrink_f(v, rc.ac);
  const double gv = sum - (double)v * b;
  if (a.emit) a.emit[(int64_t)key * (a.T.kp + 4) + c] = (float)gv;
  else a.T.v(key)[c] = upd_v(v, gv, a.p);
}
__device__ __forceinline__ void close_cols(const SegArgs& a, uint32_t key, const RowCur& rc, int c_lo, int c_hi,
                                           int c_step, double b, const double* sums) {
  const float* vrow = a.T.v(key);
  for (int c = c_lo, j = 0; c < c_hi; c += c_step, ++j) close_col(a, key, rc, c, vrow[c], b, sums[j]);
}
__device__ __forceinline__ void close_hdr(const SegArgs& a, uint32_t key, const RowCur& rc, double gw) {
  const int kp = a.T.kp;
  if (a.emit) {
    *reinterpret_cast<float2*>(a.emit + (int64_t)key * (kp + 4) + kp) = make_float2((float)gw, 1.f);
  } else {
    store_hdr(a.T, key, next_hdr(upd_w(rc.w, gw, a.p), a.p));
  }
}

constexpr int kStatLd = 8;     // block 0's stats loads in flight per thread
constexpr int kCombLanes = 16;  // lanes per range (lane f: factor columns f, f + kCombLanes, ...)
constexpr int kCombCols = 10;  // long-run columns a lane sums at once (even; W = kp + 2: k = 8 in one pass)
__global__ __launch_bounds__(kBlock) void k_segment_combine(SegArgs a, const double2* __restrict__ loss_part,
                                                            int64_t n_loss_blocks, int64_t n_ucnt,
                                                            double* __restrict__ stats_out) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kp = a.T.kp;
  const int64_t W = kp + 2;
  const int64_t N = a.n_dev ? a.n_dev[0] : a.N;
  const int64_t nranges = (N + a.L - 1) / a.L;
  __shared__ double run_sum[kBlock / 64][258];  // one long run's summed piece per wave (kp <= 256)
  if (blockIdx.x == 0) {
    __shared__ double rl[kBlock], rc[kBlock], ru[kBlock];
    double l = 0.0, c = 0.0, u = 0.0;
    // each thread's partials in index order as ever, their loads issued kStatLd at a time from
    // clamped addresses (a plain loop waits one memory round trip per element: this block closed
    // the kernel 20-30 us after the others)
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
    // update blocks that held entries (a device count leaves the grid's tail without any)
    const int64_t per_blk = (int64_t)kWaveEnt * (kBlock / 64);
    const int64_t nu = a.n_dev ? min(n_ucnt, (N + per_blk - 1) / per_blk) : n_ucnt;
    for (int64_t i0 = tid; i0 < nu; i0 += kStatLd * kBlock) {
      uint32_t v[kStatLd];
#pragma unroll
      for (int j = 0; j < kStatLd; ++j) {
        const int64_t i = i0 + j * kBlock;
        v[j] = a.ucnt[i < nu ? i : nu - 1];
      }
#pragma unroll
      for (int j = 0; j < kStatLd; ++j) u += i0 + j * kBlock < nu ? (double)v[j] : 0.0;
    }
    if (a.n_dev && tid == 0) u += (double)a.n_dev[1];  // the singleton rows the forward updated
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
  // kCombLanes lanes per range
  const int64_t chunk = ((int64_t)blockIdx.x * kBlock + tid) / kCombLanes;  // range index
  const int f = tid & (kCombLanes - 1);
  const int64_t L = a.L;
  bool owner = false, two = false;
  uint32_t key = 0;
  if (chunk < nranges) {
    const int64_t p0 = chunk * L;
    const int64_t p1 = p0 + L < N ? p0 + L : N;
    if (p1 < N) {
      // every key the two tests need, loaded together (clamped addresses: no load waits behind
      // another's comparison)
      const int64_t p2 = (chunk + 2) * L;
      const uint32_t kl = a.skeys[p1 - 1], kn = a.skeys[p1], kf = a.skeys[p0];
      const uint32_t kb = a.skeys[p0 > 0 ? p0 - 1 : 0], k2 = a.skeys[p2 < N ? p2 : N - 1];
      key = kl;
      // the range's last run continues into the next range and starts inside this range
      owner = kn == kl && !(kf == kl && p0 > 0 && kb == kl);
      // common case: the run ends inside the next range -> its two partials
      two = owner && !(p2 < N && k2 == kl);
    }
  }
  if (owner && two) {
    const double* pt = a.part + (chunk * 2 + 1) * W;
    const double* ph = a.part + ((chunk + 1) * 2) * W;
    // the two pieces' scalars and first column, the row's header and V column: one round trip
    const int cf = f < kp ? f : kp - 1;
    const double bt = pt[kp + 1], bh = ph[kp + 1], wt = pt[0], wh = ph[0];
    const double st = pt[1 + cf], sh = ph[1 + cf];
    const float vf = a.T.v(key)[cf];
    const RowCur rc = row_current(a, key);
    const double b = bt + bh;
    if (f < kp) close_col(a, key, rc, f, vf, b, st + sh);
    for (int c = f + kCombLanes; c < kp; c += kCombLanes) {
      const double sm = pt[1 + c] + ph[1 + c];
      close_cols(a, key, rc, c, c + 1, 1, b, &sm);
    }
    if (f == 0) close_hdr(a, key, rc, wt + wh);
  }
  // long runs (hot features): one wave per run, lanes over the factor columns, range order
  uint64_t owners = __ballot(owner && !two && f == 0);
  while (owners) {
    const int l = __ffsll((unsigned long long)owners) - 1;
    owners &= owners - 1;
    const int64_t c0 = __shfl(chunk, l);
    const uint32_t k0 = __shfl(key, l);
    // end of the run: first range after c0 whose first key differs
    int64_t cend = c0 + 1;
    for (;;) {
      const int64_t c = cend + lane;
      const bool cont = c < nranges && a.skeys[c * L] == k0;
      const uint64_t m = __ballot(cont);
      if (m == ~0ull) {
        cend += 64;
        continue;
      }
      cend += __ffsll((unsigned long long)~m) - 1;
      break;
    }
    // the run's pieces = the owner range's tail + the head pieces of ranges c0+1 .. cend-1, each a
    // row of W = kp + 2 doubles [g_w | sum S*x*r (kp) | sum x*x*r].  Lane l sums the pieces of
    // ranges c0+1+l, +64, ... kCombCols columns at a time (a piece's columns are contiguous, loaded
    // unconditionally from clamped addresses: one round trip per 64 ranges), then a fixed xor tree
    // over the 64 lanes, then the tail: a fixed order, so the step stays bitwise reproducible.
    for (int col0 = 0; col0 < (int)W; col0 += kCombCols) {
      double s[kCombCols];
#pragma unroll
      for (int j = 0; j < kCombCols; ++j) s[j] = 0.0;
      for (int64_t c = c0 + 1 + lane; c < cend; c += 64) {
        const double* pr = a.part + (c * 2) * W;
#pragma unroll
        for (int j = 0; j < kCombCols / 2; ++j) {
          const int cc = col0 + 2 * j;
          const double2 v = *reinterpret_cast<const double2*>(pr + (cc < (int)W ? cc : (int)W - 2));
          s[2 * j] += cc < (int)W ? v.x : 0.0;
          s[2 * j + 1] += cc < (int)W ? v.y : 0.0;
        }
      }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1)
#pragma unroll
        for (int j = 0; j < kCombCols; ++j) s[j] += __shfl_xor(s[j], o);
      if (lane == 0) {
#pragma unroll
        for (int j = 0; j < kCombCols; ++j)
          if (col0 + j < (int)W) run_sum[wave][col0 + j] = s[j];
      }
    }
    wave_lds_sync();
    for (int col = lane; col < (int)W; col += 64) run_sum[wave][col] = a.part[(c0 * 2 + 1) * W + col] + run_sum[wave][col];
    wave_lds_sync();
    const double gw = run_sum[wave][0], b = run_sum[wave][kp + 1];
    double sums[4];  // kp <= 256: columns lane, lane + 64, ...
    int j = 0;
    for (int col = lane; col < kp; col += 64, ++j) sums[j] = run_sum[wave][1 + col];
    const RowCur rc = row_current(a, k0);
    close_cols(a, k0, rc, lane, kp, 64, b, sums);
    if (lane == 0) close_hdr(a, k0, rc, gw);
    wave_lds_sync();  // run_sum is rewritten by the wave's next long run
  }
}

// ------------------------------------------------------------- replicated apply
// Every rank holds the whole table; the gradient sums of all ranks were all-reduced into
// grad[rows][kp + 4] = [sum g_V | sum g_w | touched | 0].  G lanes per row: the update + L1
// of SGD.scala:150-181 on touched rows (untouched rows take their L1 lazily, as always).
template <int G>
__global__ __launch_bounds__(kBlock) void k_repl_apply(TableView T, const float* __restrict__ grad, StepParams p,
                                                       uint32_t* __restrict__ blk_touched) {
  const int g = threadIdx.x % G;
  const int kp = T.kp, nq = kp >> 2, W = kp + 4;
  uint32_t touched = 0;
  for (int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / G; i < T.rows;
       i += (int64_t)gridDim.x * kBlock / G) {
    const float* gr = grad + i * W;
    const float2 wt = *reinterpret_cast<const float2*>(gr + kp);
    if (wt.y == 0.f) continue;
    touched += g == 0 ? 1u : 0u;
    const RowHdr h = *T.hdr(i);
    const bool present = h.t >= 0;
    const double ac = present ? p.cumE - h.cum : 0.0;
    float4* rec = reinterpret_cast<float4*>(T.v(i));
    for (int q = g; q < nq; q += G) {
      float4 v = present ? rec[q] : make_float4(0.f, 0.f, 0.f, 0.f);
      if (ac > 0.0) v = shrink4(v, ac);
      const float4 d = reinterpret_cast<const float4*>(gr)[q];
      rec[q] = make_float4(upd_v(v.x, d.x, p), upd_v(v.y, d.y, p), upd_v(v.z, d.z, p), upd_v(v.w, d.w, p));
    }
    if (g == 0) {
      float w = present ? h.w : 0.f;
      if (ac > 0.0) w = shrink_f(w, ac);
      store_hdr(T, i, next_hdr(upd_w(w, (double)wt.x, p), p));
    }
  }
  // the block's count (one word per block: a same-address atomic per wave serialises ~16K waves)
  __shared__ uint32_t wt[kBlock / 64];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) touched += __shfl_xor(touched, o);
  if ((threadIdx.x & 63) == 0) wt[threadIdx.x >> 6] = touched;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < kBlock / 64; ++w) t += wt[w];
    blk_touched[blockIdx.x] = t;
  }
}

// the blocks' counts summed into one fp64 stats slot (one block, fixed order)
__global__ __launch_bounds__(kBlock) void k_sum_counts(const uint32_t* __restrict__ c, int64_t n, double* __restrict__ out) {
  __shared__ uint64_t ws[kBlock / 64];
  uint64_t t = 0;
  for (int64_t i = threadIdx.x; i < n; i += kBlock) t += c[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t a = 0;
    for (int w = 0; w < kBlock / 64; ++w) a += ws[w];
    *out = (double)a;
  }
}
}  // namespace

// ------------------------------------------------------- singleton split (fm_batch_prepare)
// The sorted view of a batch -> the entries of its runs of two or more (stable: the order the
// segmented update needs) and the number of singleton runs.  One wave per chunk of 1024 sorted
// entries: count, one-block scan of the chunk counts, then each wave writes its multi entries at
// its offset in order (ballot ranks).  Integer work only: deterministic.  Each pass loads a wave's
// whole chunk at once (16 independent loads, not a round trip per row): in round 4 that made both
// passes twice as fast and the step slower, their bursts landing on the side stream's sort
// (profiles/r04_z, r04_za); once the sort's own latency chains were cut (round 5), the step is
// faster with it ("Latency chains").
constexpr int kSplitChunk = 1024;

// A wave's whole chunk of the sorted keys, loaded at once: row r's key per lane (clamped addresses,
// every load issued before any is used) and the keys just before and after the chunk; then per row
// whether the entry belongs to a run of two or more (multi) and whether it opens its run.
constexpr int kSplitRows = kSplitChunk / 64;
constexpr uint32_t kSplitNone = 0xFFFFFFFFu;
struct SplitChunk {
  uint32_t key[kSplitRows];
  uint32_t multi = 0, first = 0;  // bit r: row r's entry is multi / opens its run
};
__device__ __forceinline__ void split_chunk(const uint32_t* __restrict__ skeys, int64_t N, int64_t c, int lane,
                                            SplitChunk& sc) {
  const int64_t base = c * kSplitChunk;
#pragma unroll
  for (int r = 0; r < kSplitRows; ++r) {
    const int64_t p = base + r * 64 + lane;
    sc.key[r] = skeys[p < N ? p : N - 1];
  }
  // the keys just before and after the chunk, in one more load per lane (lane 0: before, the
  // others: after), unconditional so that it is issued with the rows' and not sunk into a branch
  const int64_t eb = lane == 0 ? (base > 0 ? base - 1 : 0) : (base + kSplitChunk < N ? base + kSplitChunk : N - 1);
  const uint32_t edge = skeys[eb];
  const uint32_t before = base > 0 ? __shfl(edge, 0) : kSplitNone;
  const uint32_t after = base + kSplitChunk < N ? __shfl(edge, 1) : kSplitNone;
#pragma unroll
  for (int r = 0; r < kSplitRows; ++r) {
    const int64_t p = base + r * 64 + lane;
    const uint32_t up = __shfl_up(sc.key[r], 1), dn = __shfl_down(sc.key[r], 1);
    const uint32_t pl = r > 0 ? __shfl(sc.key[r > 0 ? r - 1 : 0], 63) : before;
    const uint32_t nf = r + 1 < kSplitRows ? __shfl(sc.key[r + 1 < kSplitRows ? r + 1 : r], 0) : after;
    const uint32_t prev = lane == 0 ? pl : up;
    const uint32_t next = p + 1 >= N ? kSplitNone : (lane == 63 ? nf : dn);
    const bool valid = p < N;
    sc.multi |= (uint32_t)(valid && (prev == sc.key[r] || next == sc.key[r])) << r;
    sc.first |= (uint32_t)(valid && prev != sc.key[r]) << r;
  }
}

// (the split at the step's start, main stream) the first entry of every multi run also writes the
// epoch's multi tag into its row's header: the headers' t words are read for all rows of the chunk
// before any tag is written
__global__ __launch_bounds__(kBlock) void k_split_count(const uint32_t* __restrict__ skeys, int64_t N,
                                                        uint2* __restrict__ cnt, int64_t nchunks, TableView T,
                                                        int32_t epoch) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (c >= nchunks) return;  // wave-uniform
  SplitChunk sc;
  split_chunk(skeys, N, c, lane, sc);
  const uint32_t tag = sc.multi & sc.first;
  // every lane loads a t word per row, unconditionally (a guarded load waits out its round trip
  // before the next is issued): the run's row where it tags one, else row 0's (one shared line)
  int32_t tv[kSplitRows];
#pragma unroll
  for (int r = 0; r < kSplitRows; ++r) tv[r] = T.hdr((tag >> r) & 1u ? sc.key[r] : 0u)->t;
#pragma unroll
  for (int r = 0; r < kSplitRows; ++r)
    if ((tag >> r) & 1u) T.hdr(sc.key[r])->t = multi_tag(epoch, tv[r] >= 0);
  uint32_t nm = 0, ns = 0;
  const int64_t base = c * kSplitChunk;
#pragma unroll
  for (int r = 0; r < kSplitRows; ++r) {
    const bool valid = base + r * 64 + lane < N;
    const bool m = (sc.multi >> r) & 1u;
    nm += (uint32_t)__popcll(__ballot(m));
    ns += (uint32_t)__popcll(__ballot(valid && !m));
  }
  if (lane == 0) cnt[c] = make_uint2(nm, ns);
}

// one block: exclusive scan of the chunks' multi counts -> off[c]; totals -> n_out[0] (multi
// entries), n_out[1] (singleton runs).  It sits on the step's critical path (main stream, before
// the forward), so each thread loads its kSplitPer consecutive chunk counts of a round at once
// (from clamped addresses: as guarded loads they compiled to one round trip each):
// one memory round trip per 12K chunks (a 12.6M-entry batch: all of a c3 batch).  1024 threads x 12
// counts since round 5 (c3 0.852-0.856 against 0.856-0.862 ms for 256 x 48, four alternating reps,
// profiles/r05_aj); in round 3, with its loads still chained, 256 threads had been the faster block
// (profiles/r03_v13/ab).  Scanning in the count pass's last block instead (a device-scope counter, a
// release fence per block) cost 1.355 against 0.973 ms: each fence writes back the XCD's L2
// (profiles/r04_v); no scan at all, each scatter block summing the count pass's block totals before
// it, 1.025 against 0.976 ms (profiles/r04_w)
constexpr int kSplitPer = 12;
constexpr int kSplitScanNT = 1024;
__global__ __launch_bounds__(kSplitScanNT) void k_split_scan(const uint2* __restrict__ cnt, int64_t nchunks,
                                                             int64_t* __restrict__ off, int64_t* __restrict__ n_out) {
  constexpr int NW = kSplitScanNT / 64;
  __shared__ int64_t wsum[NW], ssum[NW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t carry = 0, singles = 0;
  for (int64_t b = 0; b < nchunks; b += kSplitScanNT * kSplitPer) {
    const int64_t i0 = b + (int64_t)threadIdx.x * kSplitPer;
    uint2 v[kSplitPer];
#pragma unroll
    for (int j = 0; j < kSplitPer; ++j) v[j] = cnt[i0 + j < nchunks ? i0 + j : nchunks - 1];  // clamped: one round trip
#pragma unroll
    for (int j = 0; j < kSplitPer; ++j)
      if (i0 + j >= nchunks) v[j] = make_uint2(0u, 0u);
    int64_t t = 0, sg = 0;
#pragma unroll
    for (int j = 0; j < kSplitPer; ++j) {
      t += v[j].x;
      sg += v[j].y;
    }
    int64_t incl = t;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int64_t u = __shfl_up(incl, o);
      if (lane >= o) incl += u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sg += __shfl_xor(sg, o);
    if (lane == 63) wsum[wave] = incl;
    if (lane == 0) ssum[wave] = sg;
    __syncthreads();
    int64_t wpre = 0, tot = 0, stot = 0;
    for (int w = 0; w < NW; ++w) {
      wpre += w < wave ? wsum[w] : 0;
      tot += wsum[w];
      stot += ssum[w];
    }
    int64_t run = carry + wpre + incl - t;
#pragma unroll
    for (int j = 0; j < kSplitPer; ++j) {
      if (i0 + j < nchunks) off[i0 + j] = run;
      run += v[j].x;
    }
    carry += tot;
    singles += stot;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    n_out[0] = carry;
    n_out[1] = singles;
  }
}

__global__ __launch_bounds__(kBlock) void k_split_scatter(const uint32_t* __restrict__ skeys,
                                                          const uint2* __restrict__ sents, int64_t N,
                                                          const int64_t* __restrict__ off, int64_t nchunks,
                                                          uint32_t* __restrict__ mkeys, uint2* __restrict__ ments) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  if (c >= nchunks) return;  // wave-uniform
  const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
  const int64_t base = c * kSplitChunk;
  // the chunk's payloads with its keys, all loads in one round trip (the payload rows are read
  // whole: a row of multi entries touches the same lines)
  uint2 en[kSplitRows];
#pragma unroll
  for (int r = 0; r < kSplitRows; ++r) {
    const int64_t p = base + r * 64 + lane;
    en[r] = sents[p < N ? p : N - 1];
  }
  int64_t o = off[c];
  SplitChunk sc;
  split_chunk(skeys, N, c, lane, sc);
#pragma unroll
  for (int r = 0; r < kSplitRows; ++r) {
    const bool m = (sc.multi >> r) & 1u;
    const uint64_t bm = __ballot(m);
    if (m) {
      const int64_t d = o + __popcll(bm & lt);
      mkeys[d] = sc.key[r];
      ments[d] = en[r];
    }
    o += __popcll(bm);
  }
}

void launch_split(const uint32_t* skeys, const uint2* sents, int64_t N, SplitWork& sw, uint32_t* mkeys, uint2* ments,
                  int64_t* n_out, hipStream_t st, const TableView& tag_T, int32_t epoch) {
  const int64_t nchunks = (N + kSplitChunk - 1) / kSplitChunk;
  sw.cnt.ensure_slack(sizeof(uint2) * (size_t)std::max<int64_t>(nchunks, 1));
  sw.off.ensure_slack(sizeof(int64_t) * (size_t)std::max<int64_t>(nchunks, 1));
  if (N <= 0) {
    FM_HIP_CHECK(hipMemsetAsync(n_out, 0, 2 * sizeof(int64_t), st));
    return;
  }
  const unsigned blocks = (unsigned)((nchunks + kBlock / 64 - 1) / (kBlock / 64));
  hipLaunchKernelGGL(k_split_count, dim3(blocks), dim3(kBlock), 0, st, skeys, N, sw.cnt.as<uint2>(), nchunks, tag_T,
                     epoch);
  hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(kSplitScanNT), 0, st, sw.cnt.as<uint2>(), nchunks, sw.off.as<int64_t>(), n_out);
  hipLaunchKernelGGL(k_split_scatter, dim3(blocks), dim3(kBlock), 0, st, skeys, sents, N, sw.off.as<int64_t>(), nchunks,
                     mkeys, ments);
  FM_HIP_CHECK(hipGetLastError());
}
void launch_segment_update(const TableView& T, const BatchDev& b, StepWork& w, const StepParams& p,
                           const uint32_t* skeys, const uint2* sents, int64_t n_fwd_blocks,
                           double* stats_out, hipStream_t st, float* emit, const int64_t* n_dev) {
  SegSource src{w.S.as<float>(), s_rec_floats(T.kp),
                 s_rec_yl(T.kp) ? reinterpret_cast<const float2*>(w.S.as<float>() + T.kp) : w.yl.as<float2>(),
                 s_rec_yl(T.kp) ? s_rec_floats(T.kp) / 2 : 1};
  src.n_dev = n_dev;
  launch_segment_update(T, b.nnz, src, w, p, skeys, sents, n_fwd_blocks, stats_out, st, emit);
}

void launch_segment_update(const TableView& T, int64_t N, const SegSource& src, StepWork& w, const StepParams& p,
                           const uint32_t* skeys, const uint2* sents, int64_t n_fwd_blocks, double* stats_out,
                           hipStream_t st, float* emit) {
  const int64_t L = kWaveEnt;
  const int64_t nranges = (N + L - 1) / L;
  w.part.ensure(sizeof(double) * (size_t)(nranges > 0 ? nranges : 1) * 2 * (T.kp + 2));
  const int64_t per_block = (int64_t)kWaveEnt * (kBlock / 64);
  const int64_t ublocks = (N + per_block - 1) / per_block;
  w.ucnt.ensure(sizeof(uint32_t) * (size_t)(ublocks > 0 ? ublocks : 1));
  SegArgs a;
  a.T = T;
  a.skeys = skeys;
  a.sents = sents;
  a.N = N;
  a.S = src.S;
  a.yl = src.yl;
  a.s_stride = src.s_stride;
  a.yl_stride = src.yl_stride;
  a.part = w.part.as<double>();
  a.nranges = nranges;
  a.L = L;
  a.p = p;
  a.ucnt = w.ucnt.as<uint32_t>();
  a.emit = emit;
  a.n_dev = src.n_dev;
  if (ublocks > 0) {
    const dim3 grid((unsigned)ublocks), blk(kBlock);
    with_update_cfg(T.kp, [&](auto cfg) {
      using Cfg = decltype(cfg);
      hipLaunchKernelGGL((k_segment_update<Cfg::Q, Cfg::NF, Cfg::D>), grid, blk, 0, st, a);
    });
    FM_HIP_CHECK(hipGetLastError());
  }
  int64_t cblocks = (nranges * kCombLanes + kBlock - 1) / kBlock;
  if (cblocks < 1) cblocks = 1;
  hipLaunchKernelGGL(k_segment_combine, dim3((unsigned)cblocks), dim3(kBlock), 0, st, a,
                     w.loss_part.as<double2>(), n_fwd_blocks, ublocks, stats_out);
  FM_HIP_CHECK(hipGetLastError());
}

UpdGeometry update_geometry(int kp) {
  UpdGeometry g{};
  g.wave_entries = kWaveEnt;
  g.block_entries = kWaveEnt * (kBlock / 64);
  with_update_cfg(kp, [&](auto cfg) {
    using Geo = UpdGeom<decltype(cfg)::Q, decltype(cfg)::NF>;
    g.group_entries = Geo::RL;
    g.paired = Geo::PAIR && kp == 4 * decltype(cfg)::Q;
  });
  g.comb_lanes = kCombLanes;
  g.comb_cols = kCombCols;
  g.split_chunk = kSplitChunk;
  g.scan_round_chunks = kSplitScanNT * kSplitPer;
  return g;
}

void launch_repl_apply(const TableView& T, const float* grad, const StepParams& p, uint32_t* blk_touched,
                       double* n_touched, hipStream_t st) {
  if (T.rows <= 0) {
    FM_HIP_CHECK(hipMemsetAsync(n_touched, 0, sizeof(double), st));
    return;
  }
  const int nq = T.kp / 4;
  const int G = nq <= 1 ? 1 : nq <= 2 ? 2 : nq <= 4 ? 4 : nq <= 8 ? 8 : 16;
  const unsigned grid = grid_for(T.rows * G, kBlock);  // <= kReplApplyBlocks
  switch (G) {
    case 1: hipLaunchKernelGGL(k_repl_apply<1>, dim3(grid), dim3(kBlock), 0, st, T, grad, p, blk_touched); break;
    case 2: hipLaunchKernelGGL(k_repl_apply<2>, dim3(grid), dim3(kBlock), 0, st, T, grad, p, blk_touched); break;
    case 4: hipLaunchKernelGGL(k_repl_apply<4>, dim3(grid), dim3(kBlock), 0, st, T, grad, p, blk_touched); break;
    case 8: hipLaunchKernelGGL(k_repl_apply<8>, dim3(grid), dim3(kBlock), 0, st, T, grad, p, blk_touched); break;
    default: hipLaunchKernelGGL(k_repl_apply<16>, dim3(grid), dim3(kBlock), 0, st, T, grad, p, blk_touched); break;
  }
  hipLaunchKernelGGL(k_sum_counts, dim3(1), dim3(kBlock), 0, st, blk_touched, (int64_t)grid, n_touched);
  FM_HIP_CHECK(hipGetLastError());
}

}  // namespace fmhip
