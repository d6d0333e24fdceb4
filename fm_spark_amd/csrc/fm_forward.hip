// The forward of the FM SGD step for gfx950 (MI355X), and the inference passes that share its
// kernel: k_forward and the launchers for the step's forward, the sharded owner's partial pass,
// predict and calcLossGrad.  The step as a whole: fm_device.h.
//
// MODE kTrain: the step's forward (S, {yhat, y}, loss partials).
// MODE kPartial: the sharded owner's pass (fm_shard.hip).  "Samples" are (source rank, sample)
// pairs of the entries this owner received; the output per pair is the partial vector
// sum v*x (kp fp32, S_out) and the scalars {sum v^2 x^2, sum w*x} (yl_out) instead of S / yhat / loss.
// MODE kPartial64: kPartial with the fp64 wire (fm_config.wire = FM_WIRE_FP64): the same sums stored
// unrounded, S_out as [pair][kp] doubles and yl_out as [pair] double2 (strides in those elements).
// MODE kPredict: FactorizationMachinesModel.predict (Model.scala:90-133): ids outside the table
// or absent from the model are dropped (the inner joins, :103-112), a row left without a learned
// feature scores globalBias unclamped (na.fill, :86), every other row
// least(greatest(yhat, minLabel), maxLabel) (:129-132), fp64 into pred_out.
// MODE kLossGrad: calcLossGrad's per-entry columns (Model.scala:225-233): the sample's yhat, its
// squared error, deltaWi = x and deltaVi = vfxiSum * x - (v * x) * x, fp64 from the team's fp64
// sums (a second walk over the sample's entries re-reads their rows); absent ids set the flag.
// MODE kTrainFused: kTrain, and every row whose feature has exactly one entry in the batch (a
// singleton: 92 % of a c3 batch's distinct rows) is updated here, by the sample that holds that
// entry, instead of by the segmented update (see "Singleton rows" in fm_device.h).
// MODE kSummary: a row's fp64 summary for fm_rank_* (fm_rank.hip): kPredict's entry handling (ids
// outside the table dropped, x from the batch's stream, the learned entries counted) with kPartial64's
// stores: S as [row][kp] doubles, {sum v^2 x^2, sum w*x} as a double2 and the count per row.
// MODE kEvaluate: kPredict's score of every row (the same entry handling and team shapes) subtracted
// from the row's fp64 label and reduced: each team keeps {rows, rows without a learned entry, sum e,
// sum |e|, sum e^2} of the rows it walks, in walking order; each block leaves one record, its teams'
// in team order; k_eval_fold sums a launch's records in an order that depends on their number alone.
// The score is stored as well when pred is given.
// (the modes are FwdMode, fm_internal.h; FwdOut::mode names the one a launch runs)
#include <atomic>

#include "fm_device.h"

namespace fmhip {

namespace {

constexpr int kFuseNS = 5;    // kTrainFused: singleton rows per lane group and sample that wait in LDS
constexpr int kPartialU = 4;  // sharded partial pass: passes (entries per lane) whose rows are in flight together
// The step's forward (and predict / loss-grad): 32 lanes per sample, 2 passes in flight -- the
// same 16 rows in flight per sample at k = 16 as 16 lanes x 4 passes, with fewer registers per
// lane (measured 1.196 against 1.213 ms per c3 step, 5 runs each on two boxes)
constexpr int kFwdTeam = 32, kFwdU = 2;
// k <= 8 (one or two lanes per row): 3 passes in flight, 96 rows per team-sample round -- c2 0.171 /
// 0.173 against 0.175 / 0.174 ms per step (median 0.162 against 0.165), at c5 (k = 16) slower
// (profiles/r04_o)
constexpr int kFwdUNarrow = 3;
// forward blocks at most (grid-stride over samples beyond): 8192 (four samples per team at c3, one at
// c2 / c5) against 2048 in round 5, c3 0.859-0.863 against 0.867-0.869 ms, c2 0.161-0.163 against
// 0.163-0.168, c5 0.178-0.181 against 0.182-0.185 (profiles/r05_ab, r05_ac; 1024 and 32768 slower)
constexpr int kFwdGrid = 8192;
// the evaluation's blocks at most: every block pays a barrier, a serial sum over its teams and a record
// that the one-block fold then reads, so fewer blocks than the forward's suit it.  Device time of
// "evaluate" (forward + fold) at c5 / c3, medians of 3 alternating reps (profiles/eval/grid_ab.json):
// 8192: 59 / 269 us, 4096: 51 / 275, 2048: 50 / 295, 1024: 59 / 281, 512: 87 / 453
constexpr int kEvalGrid = 4096;
// the fused forward (kTrainFused): 5 passes in flight (40 rows per sample at k = 16, so a 39-entry
// c3 sample takes one round instead of two): round 5 at 4 waves per SIMD, c3 0.869-0.872 against
// 0.878-0.883 ms for 3 passes, 4 passes slower (profiles/r05_x); round 3 had taken 3 (-2 to -4 %
// against 2, 4 slower under the 5-wave cap: profiles/r03_v7/ab)
constexpr int kFuseU = 5;

// calcLossGrad's draw for an entry whose id the model lacks (columns 4g .. 4g + 3 of k; f = -1: w)
__device__ __forceinline__ void fill_row(const FwdOut& xo, int k, int g, int64_t e, float4& v, float& w) {
  const int c = 4 * g;
  v = make_float4(c + 0 < k ? gauss_draw(xo.fill_seed, e, c + 0, xo.fill_sd) : 0.f,
                  c + 1 < k ? gauss_draw(xo.fill_seed, e, c + 1, xo.fill_sd) : 0.f,
                  c + 2 < k ? gauss_draw(xo.fill_seed, e, c + 2, xo.fill_sd) : 0.f,
                  c + 3 < k ? gauss_draw(xo.fill_seed, e, c + 3, xo.fill_sd) : 0.f);
  w = gauss_draw(xo.fill_seed, e, -1, xo.fill_sd);
}

// kLossGrad's second walk: the lane group rs of a team re-reads the rows of the sample's entries
// e0 + rs, + RPP, ... and writes calcLossGrad's per-entry columns from the team's sums a0..a3 (this
// lane's quad of vfxiSum) and yhat.
template <int GS, int RPP>
__device__ __forceinline__ void loss_grad_walk(const TableView& T, const uint32_t* __restrict__ col,
                                               const float* __restrict__ xs, int64_t e0, int64_t e1, int rs, int g,
                                               bool qok, double cumE, double yhat, double y, double a0, double a1,
                                               double a2, double a3, const FwdOut& xo) {
  const double d = yhat - y;
  const int k = T.k;
  for (int64_t e = e0 + rs; e < e1; e += RPP) {
    const uint32_t id = col[e];
    const double xd = (double)xs[e];
    const bool inr = id < (uint64_t)T.rows;
    const RowHdr h = inr ? *T.hdr(id) : RowHdr{0.f, -1, 0.0};
    float4 v = qok && inr ? reinterpret_cast<const float4*>(T.v(id))[g] : make_float4(0.f, 0.f, 0.f, 0.f);
    float w;
    current_row(h, v, w, cumE);
    if (xo.fill_sd > 0.0 && h.t < 0) fill_row(xo, k, g, e, v, w);
    if (g == 0) {
      if (h.t < 0) *xo.absent = 1;
      xo.pred[e] = yhat;    // prediction (Model.scala:221)
      xo.loss[e] = d * d;   // pow(pred - label, 2.0) (:230)
      xo.dw[e] = xd;        // deltaWi (:200)
    }
    double* out = xo.dv + e * k;  // deltaVi (:201-204), columns 4g .. 4g + 3 of k
    const int c = 4 * g;
    if (c + 0 < k) out[c + 0] = a0 * xd - ((double)v.x * xd) * xd;
    if (c + 1 < k) out[c + 1] = a1 * xd - ((double)v.y * xd) * xd;
    if (c + 2 < k) out[c + 2] = a2 * xd - ((double)v.z * xd) * xd;
    if (c + 3 < k) out[c + 3] = a3 * xd - ((double)v.w * xd) * xd;
  }
}

// What a sample gives the fused update of its singleton rows: the values the update kernel would
// read back -- S, r and yhat rounded to fp32 as stored.
struct SampleOut {
  float4 Sq;      // this lane's quad of S
  double rj, yh;  // r = yhat - y and yhat
};
// The gradient of a row whose run is the one entry x of that sample (SGD.scala:145-146 over a run of
// one entry) in the segmented update's terms, from the values it would read: t = x r (A = S t),
// b = x^2 r, gw = x yhat - y.  With upd_quad / upd_w_row the table is bit for bit the unfused step's.
struct SingleGrad { double t, b, gw; };
__device__ __forceinline__ SingleGrad single_grad(const SampleOut& so, double xd) {
  return SingleGrad{xd * so.rj, (xd * xd) * so.rj, (xd - 1.0) * so.yh + so.rj};  // gw: SGD.scala:145; SURVEY P1
}
// the row's V quad of this lane, updated
__device__ __forceinline__ float4 single_quad(float4 v_raw, float acf, float4 Sq, const SingleGrad& sg,
                                              const StepParams& sp) {
  const double A[4] = {fma((double)Sq.x, sg.t, 0.0), fma((double)Sq.y, sg.t, 0.0), fma((double)Sq.z, sg.t, 0.0),
                       fma((double)Sq.w, sg.t, 0.0)};
  return upd_quad(v_raw, acf, A, sg.b, sp);
}

// kTrainFused (kp <= 16): each lane group keeps, in LDS, the singleton rows among the entries it
// gathers (raw V quads + header with x + id; slot rs + j RPP for its j-th singleton, at most NS
// per sample) -- no global re-read -- and after the sample's reduction rewrites them updated in
// place.  Their stores go out during the next sample, once its first ids are in and before its
// first row gathers, so no gather is queued behind them; the last sample's at the end.  Every
// slot is read and written by the lanes of the group that gathered it: no barrier.
template <int GS, int TEAM, bool STASH>
struct SingletonStash {
  static_assert(!STASH || (GS <= 4 && TEAM >= 16), "the fused forward serves kp <= 16");
  static constexpr int RPP = TEAM / GS;  // entries per pass
  static constexpr int TPB = kBlock / TEAM;
  static constexpr int NS = STASH ? kFuseNS : 1;  // singleton rows a lane group keeps per sample
  static constexpr int MZ = STASH ? NS * RPP : 1;
  // the block's LDS: function-local statics, one set per fused kernel (held as reference members of
  // this struct, the same arrays cost the fused forward 2-8 VGPRs and, at k <= 8, its fourth wave)
  using LdsV = float4[STASH ? TPB : 1][MZ][STASH ? GS : 1];
  using LdsH = float4[STASH ? TPB : 1][MZ];
  using LdsId = uint32_t[STASH ? TPB : 1][MZ];
  static __device__ __forceinline__ LdsV& lds_v() { __shared__ LdsV a; return a; }
  static __device__ __forceinline__ LdsH& lds_h() { __shared__ LdsH a; return a; }
  static __device__ __forceinline__ LdsId& lds_id() { __shared__ LdsId a; return a; }
  const TableView& T;
  const int team, rs, g;
  const bool qok;
  const int span;  // header + zero pad of its 64-B granule
  int nst = 0;     // singletons of the current sample met by this lane group
  int pend = 0;    // updated rows of the previous sample waiting in slots rs + j RPP, j < pend

  __device__ __forceinline__ SingletonStash(const TableView& T_, int team_, int rs_, int g_, bool qok_)
      : T(T_), team(team_), rs(rs_), g(g_), qok(qok_), span(hdr_span(T_.kp)) {}

  // the neighbour group's count of waiting rows (call it where every lane of the team is active: a
  // shuffle from a lane outside the exec mask reads garbage)
  __device__ __forceinline__ int neighbour_pend() const { return STASH && GS >= 2 ? __shfl_xor(pend, GS) : 0; }

  // a singleton row met while gathering: raw V quad, header and id kept (the first NS), all counted;
  // the group's lanes see the same entry, so nst stays uniform across them
  __device__ __forceinline__ void keep(const RowHdr& h, float4 v, float x, uint32_t id) {
    if (nst < NS) {
      const int i = rs + nst * RPP;
      lds_v()[team][i][g] = v;
      if (g == 0) {  // the header with the entry's x in place of t (the update rewrites t)
        RowHdr hx = h;
        hx.t = __float_as_int(x);
        lds_h()[team][i] = *reinterpret_cast<const float4*>(&hx);
        lds_id()[team][i] = id;
      }
    }
    ++nst;
  }

  // pp = the neighbour group's pend, exchanged while the whole team is active (flush() itself runs
  // from two call sites: a group without an entry in the sample flushes before the entry loop, one
  // with entries inside it, so the two groups of a pair may flush at different points; each then
  // writes its own rows' V and the neighbour's headers from the count taken here, and neither
  // group's slots change before both have flushed -- a group stashes only after its own flush, and
  // only when it has entries)
  __device__ __forceinline__ void flush(int pp) {
    const int kp = T.kp;
    if constexpr (GS >= 2) {
      // paired: each updated record leaves in ONE store instruction of 2 GS lanes -- the group
      // writes its row's V, the neighbour group (rs ^ 1) that row's header granule (span <= 4 GS)
      // -- first the even groups' rows, then the odd groups' (a record written by two half-record
      // instructions costs more: DESIGN.md §5, paired row stores)
      const bool even = (rs & 1) == 0;
      const int n = pend > pp ? pend : pp;
      for (int j = 0; j < n; ++j) {
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
          const bool writer = even == (pass == 0);  // this lane writes V of its own group's row
          const int slot = (writer ? rs : rs ^ 1) + j * RPP;
          const bool live = j < (writer ? pend : pp);
          const uint32_t sid = live ? lds_id()[team][slot] : 0u;
          float* rec = T.v(sid);
          const float4 val = writer ? lds_v()[team][slot][g] : (g == 0 ? lds_h()[team][slot] : make_float4(0.f, 0.f, 0.f, 0.f));
          if (live && (writer ? qok : 4 * g < span)) st_row4(writer ? rec + 4 * g : rec + kp + 4 * g, val);
        }
      }
    } else {
      for (int j = 0; j < pend; ++j) {
        const int i = rs + j * RPP;
        float* rec = T.v(lds_id()[team][i]);
        if (qok) st_row4(rec + 4 * g, lds_v()[team][i][g]);
        for (int c = 4 * g; c < span; c += 4 * GS) st_row4(rec + kp + c, c == 0 ? lds_h()[team][i] : make_float4(0.f, 0.f, 0.f, 0.f));
      }
    }
    pend = 0;
  }

  // After the sample's reduction: the rows whose only entry in this batch belongs to this sample.
  // The row was read a moment ago (an L2 hit); the update kernel skips these runs (no row read, no
  // S gather there).
  __device__ __forceinline__ void update(const SampleOut& so, const StepParams& sp, const uint32_t* __restrict__ col,
                                         const float* __restrict__ xs, int64_t e0, int64_t e1) {
    // the stashed rows (the group's first NS singletons), updated in place in LDS
    const int zc = nst < NS ? nst : NS;
    for (int jj = 0; jj < zc; ++jj) {
      const int i = rs + jj * RPP;
      const float4 hq = lds_h()[team][i];
      const RowHdr h = *reinterpret_cast<const RowHdr*>(&hq);
      const double xd = (double)__int_as_float(h.t);  // the stash keeps x in the t word
      const float acf = pending_l1(h, sp);
      const SingleGrad sg = single_grad(so, xd);
      if (qok) lds_v()[team][i][g] = single_quad(lds_v()[team][i][g], acf, so.Sq, sg, sp);
      if (g == 0) {
        const RowHdr o = next_hdr(upd_w_row(h, acf, 0.0 + sg.gw, sp), sp);
        lds_h()[team][i] = *reinterpret_cast<const float4*>(&o);
      }
    }
    pend = zc;
    // singletons beyond the group's NS (long samples): the group walks its entries again, and
    // rows past the first NS singletons are read again (nobody else reads or writes a singleton
    // row in this step) and updated straight away
    const int kp = T.kp;
    int seen = 0;
    for (int64_t e = e0 + rs; nst > NS && e < e1; e += RPP) {
      const uint32_t id = col[e];
      const RowHdr h = *T.hdr(id);
      if (is_multi(h.t, sp.epoch)) continue;
      if (++seen <= NS) continue;  // stashed
      const float4 vq = qok ? reinterpret_cast<const float4*>(T.v(id))[g] : make_float4(0.f, 0.f, 0.f, 0.f);
      const double xd = (double)xs[e];
      const float acf = pending_l1(h, sp);
      float* rec = T.v(id);
      const SingleGrad sg = single_grad(so, xd);
      if (qok) st_row4(rec + 4 * g, single_quad(vq, acf, so.Sq, sg, sp));
      for (int i = 4 * g; i < span; i += 4 * GS) {  // the header and the zero pad of its granule
        float4 hq = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i == 0) {
          const RowHdr o = next_hdr(upd_w_row(h, acf, 0.0 + sg.gw, sp), sp);
          hq = *reinterpret_cast<const float4*>(&o);
        }
        st_row4(rec + kp + i, hq);
      }
    }
  }
};

// The fused forward at 4 waves per SIMD (107 VGPRs, no spill).  Round 3 measured 5 waves (96
// VGPRs, a few spilled) faster: c3 step 0.98 against 1.03 ms (profiles/r03_v9/ab, r03_v10/ab);
// with the small kernels' latency chains cut (round 5) the spills cost more than the fifth wave
// buys: 0.881-0.882 against 0.892-0.894 ms, five alternating reps (profiles/r05_w2).  6 waves (80
// VGPRs, more spills) measured 1.066 in round 3.  The other modes keep the compiler's choice.
template <int MODE, int GS>
constexpr int fwd_min_waves() { return MODE == kTrainFused && GS == 4 ? 4 : 1; }  // k = 9..16 (smaller
// k: the stash's LDS holds the block count below 4 waves anyway)

// Per team and sample: chunk prologue (partial modes) -> the entries' rows loaded and accumulated,
// U passes in flight -> team reduction -> the mode's epilogue.
template <int GS, int TEAM, int MODE, int U>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(fwd_min_waves<MODE, GS>())))
void k_forward(TableView T, const int64_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
               const uint2* __restrict__ ent, const float* __restrict__ xs, const double* __restrict__ label, int64_t B,
               double w0, double cumE, float* __restrict__ S_out, float2* __restrict__ yl_out, int64_t sstr, int64_t ystr,
               double2* __restrict__ loss_part, FwdOut xo) {
  constexpr bool PARTIAL = MODE == kPartial || MODE == kPartial64;
  constexpr bool STASH = MODE == kTrainFused;
  constexpr bool SUMMARY = MODE == kSummary;  // predict's entries, the fp64 partial pass's stores
  constexpr bool SCORE = MODE == kPredict || MODE == kEvaluate;  // predict's entries and its score per row
  using Stash = SingletonStash<GS, TEAM, STASH>;
  constexpr int RPP = TEAM / GS;  // entries per pass
  constexpr int TPB = kBlock / TEAM;
  const int tid = threadIdx.x;
  const int tl = tid % TEAM;
  const int g = tl % GS;
  const int rs = tl / GS;
  const int kp = T.kp;
  const bool qok = g * 4 < kp;
  double loss_acc = 0.0, nloss = 0.0;
  // kEvaluate: the record of each team's rows, kept by its lane tl == 0 -- in LDS: the five fp64 sums
  // held in registers across the sample loop took the kernel from kPredict's 56-72 VGPRs to 74-92, two
  // waves per SIMD fewer (or, held to kPredict's occupancy, were spilled to scratch).  Only that lane
  // reads or writes its team's slot: no barrier until the block's reduction.
  __shared__ double ev_team[MODE == kEvaluate ? kEvalRec : 1][MODE == kEvaluate ? TPB : 1];
  if constexpr (MODE == kEvaluate) {
    if (tl == 0) {
#pragma unroll
      for (int c = 0; c < kEvalRec; ++c) ev_team[c][tid / TEAM] = 0.0;
    }
  }

  // ---- chunk prologue.  kPartial over one chunk of the pairs: the chunk's pairs numbered source by source
  __shared__ int64_t ch_base[PARTIAL ? kMaxChunkSources + 1 : 1], ch_start[PARTIAL ? kMaxChunkSources : 1];
  const bool chunked = PARTIAL && xo.ch_C > 1;
  int64_t Bl = B;
  if (chunked) {
    if (tid == 0) {
      int64_t acc = 0;
      for (int r = 0; r < xo.ch_R; ++r) {
        const int64_t p0 = xo.ch_off[r], P = xo.ch_off[r + 1] - p0;
        const int64_t lo = P * xo.ch_c / xo.ch_C, hi = P * (xo.ch_c + 1) / xo.ch_C;
        ch_start[r] = p0 + lo;
        ch_base[r] = acc;
        acc += hi - lo;
      }
      ch_base[xo.ch_R] = acc;
    }
    __syncthreads();
    Bl = ch_base[xo.ch_R];
  }

  Stash stash(T, tid / TEAM, rs, g, qok);

  for (int64_t sl = (int64_t)blockIdx.x * TPB + tid / TEAM; sl < Bl; sl += (int64_t)gridDim.x * TPB) {
    int64_t s = sl;
    if (chunked) {
      int r = 0;
      while (sl >= ch_base[r + 1]) ++r;
      s = ch_start[r] + (sl - ch_base[r]);
    }
    const int64_t e0 = row_ptr[s], e1 = row_ptr[s + 1];
    // the fused update needs the label in every lane after the reduction: its load is issued now,
    // with the sample's first loads, not behind the reduction
    const double ys = MODE == kTrainFused ? label[s] : 0.0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, vv = 0.0, wx = 0.0;
    uint32_t npres = 0;  // kPredict: learned entries of the sample (this lane's share)
    const int pp_s = stash.neighbour_pend();  // taken here, where every lane of the team is active
    if (STASH) {
      stash.nst = 0;
      if (e0 + rs >= e1) stash.flush(pp_s);  // no entry of this sample for the lane group: nothing to wait behind
    }
    // ---- the sample's entries: U passes of RPP entries loaded, then accumulated
    for (int64_t eb = e0 + rs; eb < e1; eb += U * RPP) {
      uint32_t id[U];
      float x[U];
      bool ok[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const int64_t e = eb + j * RPP;
        ok[j] = e < e1;
        if constexpr (MODE == kTrainFused) {
          // (the fused forward issues these guarded loads together already; under its register
          // budget the unguarded form below came out c3 within the noise, slower: profiles/r05_q)
          id[j] = ok[j] ? col[e] : 0u;
          x[j] = ok[j] ? xs[e] : 0.f;
        } else {
          // loaded from a clamped index, unguarded (eb < e1 here): every id and x of the round in
          // flight at once (a guarded load, or one behind the predict's id test, waits out its round
          // trip first -- the partial pass's were issued in three groups: R = 8 owner forward 0.356
          // -> 0.277 ms, profiles/r05_q)
          const int64_t ec = ok[j] ? e : e1 - 1;
          const uint32_t idl = col[ec];
          // the batch's x stream (4 B per entry); the partial pass's entries carry x themselves
          const float xl = PARTIAL ? __uint_as_float(ent[ec].y) : xs[ec];
          id[j] = ok[j] ? idl : 0u;
          if (SCORE || SUMMARY) ok[j] = ok[j] && id[j] < (uint64_t)T.rows;
          x[j] = ok[j] ? xl : 0.f;
        }
      }
      if (STASH && eb == e0 + rs) stash.flush(pp_s);  // the previous sample's rows: ids in, gathers not yet issued
      RowHdr h[U];
      float4 v[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        // loss-grad with the fill takes ids beyond the table (the left outer join): absent rows
        if (ok[j] && (MODE != kLossGrad || id[j] < (uint64_t)T.rows)) {
          h[j] = *T.hdr(id[j]);
          v[j] = qok ? reinterpret_cast<const float4*>(T.v(id[j]))[g] : make_float4(0.f, 0.f, 0.f, 0.f);
        } else {
          h[j] = RowHdr{0.f, -1, 0.0};
          v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
#pragma unroll
      for (int j = 0; j < U; ++j) {
        // a singleton row (untagged), updated by this sample after its reduction
        if (STASH && ok[j] && !is_multi(h[j].t, xo.sp.epoch)) stash.keep(h[j], v[j], x[j], id[j]);
      }
#pragma unroll
      for (int j = 0; j < U; ++j) {
        float w;
        if ((SCORE || PARTIAL || SUMMARY) && g == 0 && h[j].t >= 0) ++npres;
        current_row(h[j], v[j], w, cumE);
        if (MODE == kLossGrad && xo.fill_sd > 0.0 && ok[j] && h[j].t < 0) fill_row(xo, T.k, g, eb + j * RPP, v[j], w);
        const double xd = x[j];
        // vfxi = v * x (Model.scala:179), VectorSum over the sample (:191)
        a0 += (double)v[j].x * xd; a1 += (double)v[j].y * xd;
        a2 += (double)v[j].z * xd; a3 += (double)v[j].w * xd;
        // vi2xi2 = (sum_f v_f^2) * x * x (Model.scala:256-258), this lane's factors
        const double v2 = (double)v[j].x * v[j].x + (double)v[j].y * v[j].y + (double)v[j].z * v[j].z +
                          (double)v[j].w * v[j].w;
        vv += v2 * xd * xd;
        if (g == 0) wx += (double)w * xd;  // wixi (Model.scala:178)
      }
    }
    // ---- team reduction: sum the entry slots (lanes with equal g), then the whole team for the scalars
#pragma unroll
    for (int o = GS; o < TEAM; o <<= 1) {
      a0 += __shfl_xor(a0, o); a1 += __shfl_xor(a1, o);
      a2 += __shfl_xor(a2, o); a3 += __shfl_xor(a3, o);
    }
#pragma unroll
    for (int o = 1; o < TEAM; o <<= 1) {
      vv += __shfl_xor(vv, o);
      wx += __shfl_xor(wx, o);
      if (SCORE || PARTIAL || SUMMARY) npres += __shfl_xor(npres, o);
    }
    // ---- the mode's epilogue
    if (PARTIAL || SUMMARY) {  // vectors [pair][kp] in S_out, scalars {sum v^2 x^2, sum w x} in yl_out
      if constexpr (MODE == kPartial64 || SUMMARY) {  // the fp64 wire: two 16-B stores per lane, one for the scalars
        if (rs == 0 && qok) {
          double2* so = reinterpret_cast<double2*>(reinterpret_cast<double*>(S_out) + s * sstr + g * 4);
          so[0] = make_double2(a0, a1);
          so[1] = make_double2(a2, a3);
        }
        if (tl == 0) reinterpret_cast<double2*>(yl_out)[s * ystr] = make_double2(vv, wx);
      } else {
        if (rs == 0 && qok)
          *reinterpret_cast<float4*>(S_out + s * sstr + g * 4) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
        if (tl == 0) yl_out[s * ystr] = make_float2((float)vv, (float)wx);
      }
      if (tl == 0) {
        if (xo.pcount) xo.pcount[s] = npres;
      }
      continue;
    }
    double ss = qok ? a0 * a0 + a1 * a1 + a2 * a2 + a3 * a3 : 0.0;
#pragma unroll
    for (int o = 1; o < GS; o <<= 1) ss += __shfl_xor(ss, o);
    // sumVx + wixiSum + w0 (Model.scala:221, :260-262)
    const double yhat = 0.5 * (ss - vv) + wx + w0;
    if (MODE == kPredict) {
      if (tl == 0) xo.pred[s] = npres == 0 ? w0 : fmin(fmax(yhat, xo.lo), xo.hi);
      continue;
    }
    if constexpr (MODE == kEvaluate) {
      // predict's score against the row's label, into this thread's record (a row without entries is a
      // row: it scores w0); the stored prediction is the one that was subtracted
      if (tl == 0) {
        EvalAcc row;
        const double p = eval_row(row, yhat, npres != 0, w0, xo.lo, xo.hi, label[s]);
        if (xo.pred) xo.pred[s] = p;
#pragma unroll
        for (int c = 0; c < kEvalRec; ++c) ev_team[c][tid / TEAM] += row.v[c];
      }
      continue;
    }
    if (MODE == kLossGrad) {
      loss_grad_walk<GS, RPP>(T, col, xs, e0, e1, rs, g, qok, cumE, yhat, label[s], a0, a1, a2, a3, xo);
      continue;
    }
    if (rs == 0 && qok)
      *reinterpret_cast<float4*>(S_out + s * sstr + g * 4) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
    if constexpr (STASH) {
      const float r32 = (float)(yhat - ys), yh32 = (float)yhat;
      const SampleOut so{make_float4((float)a0, (float)a1, (float)a2, (float)a3), (double)r32, (double)yh32};
      stash.update(so, xo.sp, col, xs, e0, e1);
    }
    if (tl == 0) {
      const double y = label[s];
      // r = pred - label in fp64 (SGD.scala:146), rounded once: relative error 2^-24 of r itself
      yl_out[s * ystr] = make_float2((float)(yhat - y), (float)yhat);
      if (e1 > e0) {
        const double d = yhat - y;
        loss_acc += d * d;  // pow(pred - label, 2.0), Model.scala:230
        nloss += 1.0;
      }
    }
  }
  if (STASH) stash.flush(stash.neighbour_pend());  // the last sample's rows (the whole wave active)
  if constexpr (MODE == kTrain || MODE == kTrainFused) block_loss_partial(loss_acc, nloss, loss_part);
  // the block's record: its teams' sums in team order (it goes where the step's loss partial goes:
  // loss_part is [blocks][kEvalRec] doubles here)
  if constexpr (MODE == kEvaluate) {
    __syncthreads();
    if (tid == 0) {
      double* out = reinterpret_cast<double*>(loss_part) + (int64_t)blockIdx.x * kEvalRec;
#pragma unroll
      for (int c = 0; c < kEvalRec; ++c) {
        double sum = 0.0;
        for (int t = 0; t < TPB; ++t) sum += ev_team[c][t];
        out[c] = sum;
      }
    }
  }
}

// The n per-block records of an evaluation launch -> one record (one block): thread t adds the records
// t, t + kBlock, ... in that order, then the block reduction.  The order depends on n alone.
__global__ __launch_bounds__(kBlock) void k_eval_fold(const double* __restrict__ part, int64_t n, double* __restrict__ out) {
  EvalAcc a;
#pragma unroll 8
  for (int64_t i = threadIdx.x; i < n; i += kBlock) {  // (unrolled: the records' loads in flight together, added in order)
#pragma unroll
    for (int c = 0; c < kEvalRec; ++c) a.v[c] += part[i * kEvalRec + c];
  }
  block_eval_partial(a, out);
}

// The suite's seam (fm_internal.h, set_forward_grid_cap): the block cap in force, 0 = kFwdGrid, and
// the launches made under a cap.
std::atomic<int64_t> g_grid_cap{0};
std::mutex g_log_mu;  // a group's ranks launch from their own threads
std::vector<FwdLaunchRec> g_log;
int64_t g_logged = 0;

void log_launch(const FwdLaunchRec& r) {
  std::lock_guard<std::mutex> lk(g_log_mu);
  if ((int)g_log.size() < kFwdLogCap) g_log.push_back(r);
  ++g_logged;
}

// The one launch of k_forward: the arguments each mode takes.
template <int GS, int TEAM, int MODE, int U>
void launch_fwd_m(const TableView& T, const BatchDev& b, StepWork& w, const StepParams& p, hipStream_t st,
                  int64_t* nblk, float* partial_out, FwdOut xo) {
  constexpr bool PARTIAL = MODE == kPartial || MODE == kPartial64, TRAIN = MODE == kTrain || MODE == kTrainFused;
  constexpr int TPB = kBlock / TEAM;
  int64_t blocks = (b.n_rows + TPB - 1) / TPB;
  const int64_t cap = g_grid_cap.load(std::memory_order_relaxed);  // the suite's seam; 0 = the tuned grid
  const int64_t grid = cap > 0 ? cap : (MODE == kEvaluate ? kEvalGrid : kFwdGrid);
  if (blocks > grid) blocks = grid;
  if (blocks < 1) blocks = 1;
  *nblk = blocks;
  if (cap > 0) log_launch(FwdLaunchRec{MODE, GS, TEAM, U, PARTIAL ? xo.ch_c : 0, PARTIAL ? xo.ch_C : 1, blocks, b.n_rows});
  float* S_out = nullptr;
  float2* yl_out = nullptr;
  int64_t sstr = T.kp, ystr = 1;
  double2* loss_part = nullptr;
  if (PARTIAL) {
    // [n_rows][kp] fp32 vectors, then [n_rows] float2 scalars (xo: the present counts); the fp64
    // wire: [n_rows][kp] doubles, then [n_rows] double2
    S_out = partial_out;
    yl_out = MODE == kPartial64 ? reinterpret_cast<float2*>(reinterpret_cast<double*>(partial_out) + b.n_rows * T.kp)
                                : reinterpret_cast<float2*>(partial_out + b.n_rows * T.kp);
  }
  if (MODE == kSummary) {  // the fp64 wire's layout in xo.summary
    S_out = reinterpret_cast<float*>(xo.summary);
    yl_out = reinterpret_cast<float2*>(xo.summary + b.n_rows * T.kp);
  }
  if (TRAIN) {
    w.loss_part.ensure(sizeof(double2) * blocks);
    S_out = w.S.as<float>();
    yl_out = s_rec_yl(T.kp) ? reinterpret_cast<float2*>(w.S.as<float>() + T.kp) : w.yl.as<float2>();
    sstr = s_rec_floats(T.kp);
    ystr = s_rec_yl(T.kp) ? (int64_t)s_rec_floats(T.kp) / 2 : (int64_t)1;
    loss_part = w.loss_part.as<double2>();
    if (MODE == kTrainFused) xo.sp = p;  // the singleton rows' updates in the forward
  }
  if (MODE == kEvaluate) {  // one record per block (every block writes its own, also one without rows)
    // (through the kernel's loss_part argument: a field more in FwdOut moved the scalar registers of
    // the loss-grad instantiations)
    w.eval_part.ensure_slack(sizeof(double) * kEvalRec * (size_t)blocks);
    loss_part = w.eval_part.as<double2>();
  }
  // the partial pass's entries carry x themselves; labels: the step, loss-grad and the evaluation
  hipLaunchKernelGGL((k_forward<GS, TEAM, MODE, U>), dim3((unsigned)blocks), dim3(kBlock), 0, st, T,
                     b.row_ptr.as<int64_t>(), b.col.as<uint32_t>(), b.ent.as<uint2>(),
                     PARTIAL ? nullptr : b.xs.as<float>(),
                     TRAIN || MODE == kLossGrad || MODE == kEvaluate ? b.label.as<double>() : nullptr,
                     b.n_rows, p.w0, p.cumE, S_out, yl_out, sstr, ystr, loss_part, xo);
}

// xo.mode -> the kernel of that mode for one team shape
template <int GS, int TEAM, int U>
void launch_fwd_t(const TableView& T, const BatchDev& b, StepWork& w, const StepParams& p, hipStream_t st,
                  int64_t* nblk, float* partial_out, const FwdOut& xo) {
  switch (xo.mode) {
    case kPartial64:
      // (only the partial pass's own shapes carry the wide store: the step's U never reaches here)
      if constexpr (U == kPartialU) return launch_fwd_m<GS, TEAM, kPartial64, U>(T, b, w, p, st, nblk, partial_out, xo);
      else FM_REQUIRE(false, "the fp64 partial store serves the partial pass only");
      break;
    case kPartial: return launch_fwd_m<GS, TEAM, kPartial, U>(T, b, w, p, st, nblk, partial_out, xo);
    case kPredict: return launch_fwd_m<GS, TEAM, kPredict, U>(T, b, w, p, st, nblk, partial_out, xo);
    case kSummary:
      // (predict's team shapes only: the partial pass's narrow teams never summarise)
      if constexpr (TEAM >= kFwdTeam) return launch_fwd_m<GS, TEAM, kSummary, U>(T, b, w, p, st, nblk, partial_out, xo);
      else FM_REQUIRE(false, "the row summary takes predict's team shapes");
      break;
    case kEvaluate:
      // (predict's team shapes only, as the row summary)
      if constexpr (TEAM >= kFwdTeam) return launch_fwd_m<GS, TEAM, kEvaluate, U>(T, b, w, p, st, nblk, partial_out, xo);
      else FM_REQUIRE(false, "the evaluation takes predict's team shapes");
      break;
    case kLossGrad: return launch_fwd_m<GS, TEAM, kLossGrad, U>(T, b, w, p, st, nblk, partial_out, xo);
    case kTrainFused:
      if constexpr (GS <= 4 && TEAM >= 16) return launch_fwd_m<GS, TEAM, kTrainFused, kFuseU>(T, b, w, p, st, nblk, partial_out, xo);
      else FM_REQUIRE(false, "the fused forward serves kp <= 16");
      break;
    default: return launch_fwd_m<GS, TEAM, kTrain, U>(T, b, w, p, st, nblk, partial_out, xo);
  }
}

// The sharded owner's partial pass sees short segments (about z / R entries per pair): its team
// is sized so one round of U = 4 passes covers a segment, instead of 16 lanes per segment.
template <int GS>
void launch_partial_t(const TableView& T, const BatchDev& b, StepWork& w, const StepParams& p, hipStream_t st,
                      int64_t* nblk, float* partial_out, const FwdOut& xo) {
  const double avg = b.n_rows > 0 ? (double)b.nnz / (double)b.n_rows : 0.0;
  if (GS <= 16 && avg <= 4.0) launch_fwd_t<GS, GS, kPartialU>(T, b, w, p, st, nblk, partial_out, xo);
  else if (GS <= 16 && avg <= 8.0) launch_fwd_t<GS, (2 * GS > 16 ? 16 : 2 * GS), kPartialU>(T, b, w, p, st, nblk, partial_out, xo);
  else launch_fwd_t<GS, (GS > 16 ? GS : 16), kPartialU>(T, b, w, p, st, nblk, partial_out, xo);
}

}  // namespace

void set_forward_grid_cap(int64_t blocks) { g_grid_cap.store(blocks > 0 ? blocks : 0, std::memory_order_relaxed); }

void clear_forward_log() {
  std::lock_guard<std::mutex> lk(g_log_mu);
  g_log.clear();
  g_logged = 0;
}

int read_forward_log(FwdLaunchRec* out, int cap) {
  std::lock_guard<std::mutex> lk(g_log_mu);
  for (int i = 0; out && i < cap && i < (int)g_log.size(); ++i) out[i] = g_log[i];
  return (int)g_logged;
}

FwdConsts forward_consts() { return FwdConsts{kFwdGrid, kBlock, kFuseNS, kFuseU}; }

void launch_forward(const TableView& T, const BatchDev& b, StepWork& w, const StepParams& p, hipStream_t st,
                    int64_t* nblk, float* partial_out, const FwdOut* pred, bool partial_wide) {
  // the mode, stated once: a partial pass by its output buffer, else what the caller's FwdOut names
  // (kTrain without one)
  FwdOut xo = pred ? *pred : FwdOut{};
  if (partial_out) xo.mode = partial_wide ? kPartial64 : kPartial;
  const int nq = T.kp / 4;
  constexpr int TM = kFwdTeam, TU = kFwdU;
  FM_REQUIRE(nq <= 64, "dimFactorization > 256 is not supported");
  if (nq > 32) launch_fwd_t<64, 64, kPartialU>(T, b, w, p, st, nblk, partial_out, xo);
  else if (nq > 16) launch_fwd_t<32, 32, kPartialU>(T, b, w, p, st, nblk, partial_out, xo);
  else if (partial_out) {
    if (nq <= 1) launch_partial_t<1>(T, b, w, p, st, nblk, partial_out, xo);
    else if (nq <= 2) launch_partial_t<2>(T, b, w, p, st, nblk, partial_out, xo);
    else if (nq <= 4) launch_partial_t<4>(T, b, w, p, st, nblk, partial_out, xo);
    else if (nq <= 8) launch_partial_t<8>(T, b, w, p, st, nblk, partial_out, xo);
    else launch_partial_t<16>(T, b, w, p, st, nblk, partial_out, xo);
  } else if (nq <= 1) launch_fwd_t<1, TM, kFwdUNarrow>(T, b, w, p, st, nblk, partial_out, xo);
  else if (nq <= 2) launch_fwd_t<2, TM, kFwdUNarrow>(T, b, w, p, st, nblk, partial_out, xo);
  else if (nq <= 4) launch_fwd_t<4, (TM < 4 ? 4 : TM), TU>(T, b, w, p, st, nblk, partial_out, xo);
  else if (nq <= 8) launch_fwd_t<8, (TM < 8 ? 8 : TM), TU>(T, b, w, p, st, nblk, partial_out, xo);
  else launch_fwd_t<16, (TM < 16 ? 16 : TM), TU>(T, b, w, p, st, nblk, partial_out, xo);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_predict(const TableView& T, const BatchDev& b, double cumE, double w0, double lo, double hi,
                    double* pred, hipStream_t st) {
  FM_REQUIRE(T.shard_count == 1, "fm_predict needs the whole table (shard_count == 1)");
  if (b.n_rows <= 0) return;
  StepParams p{};
  p.cumE = cumE;
  p.w0 = w0;
  FwdOut xo{};
  xo.mode = kPredict;
  xo.lo = lo;
  xo.hi = hi;
  xo.pred = pred;
  StepWork unused;
  int64_t nblk = 0;
  launch_forward(T, b, unused, p, st, &nblk, nullptr, &xo);
}

void launch_eval_fold(const double* part, int64_t n_blocks, double* out, hipStream_t st) {
  hipLaunchKernelGGL(k_eval_fold, dim3(1), dim3(kBlock), 0, st, part, n_blocks, out);
  FM_HIP_CHECK(hipGetLastError());
}

int64_t launch_evaluate(const TableView& T, const BatchDev& b, StepWork& w, double cumE, double w0, double lo, double hi,
                        double* pred, hipStream_t st) {
  FM_REQUIRE(T.shard_count == 1, "fm_evaluate needs the whole table (shard_count == 1)");
  FM_REQUIRE(b.n_rows > 0, "nothing to evaluate");
  StepParams p{};
  p.cumE = cumE;
  p.w0 = w0;
  FwdOut xo{};
  xo.mode = kEvaluate;
  xo.lo = lo;
  xo.hi = hi;
  xo.pred = pred;
  int64_t nblk = 0;
  launch_forward(T, b, w, p, st, &nblk, nullptr, &xo);
  return nblk;
}

void launch_summary(const TableView& T, const BatchDev& b, double cumE, double* summary, uint32_t* present,
                    hipStream_t st) {
  FM_REQUIRE(T.shard_count == 1, "fm_rank needs the whole table (shard_count == 1)");
  if (b.n_rows <= 0) return;
  StepParams p{};
  p.cumE = cumE;
  FwdOut xo{};
  xo.mode = kSummary;
  xo.summary = summary;
  xo.pcount = present;
  StepWork unused;
  int64_t nblk = 0;
  launch_forward(T, b, unused, p, st, &nblk, nullptr, &xo);
}

void launch_loss_grad(const TableView& T, const BatchDev& b, double cumE, double w0, double* pred, double* loss,
                      double* dw, double* dv, int32_t* absent_flag, hipStream_t st, double fill_sd, uint64_t fill_seed) {
  FM_REQUIRE(T.shard_count == 1, "fm_loss_grad needs the whole table (shard_count == 1)");
  if (b.n_rows <= 0) return;
  StepParams p{};
  p.cumE = cumE;
  p.w0 = w0;
  FwdOut xo{};
  xo.mode = kLossGrad;
  xo.pred = pred;
  xo.loss = loss;
  xo.dw = dw;
  xo.dv = dv;
  xo.absent = absent_flag;
  xo.fill_sd = fill_sd;
  xo.fill_seed = fill_seed;
  StepWork unused;
  int64_t nblk = 0;
  launch_forward(T, b, unused, p, st, &nblk, nullptr, &xo);
}

}  // namespace fmhip
