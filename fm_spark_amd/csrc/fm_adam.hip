// The lazy AdamW rule of the wave-per-window update stage (fm_window.h) for gfx950 (MI355X):
// fm_config.optimizer == FM_OPT_ADAM (Kingma & Ba, ICLR 2015; the decoupled decay of Loshchilov & Hutter, ICLR
// 2019).  The stage, its geometry, its scratch and the state's zeroing are FTRL's (fm_ftrl.hip); an SGD, AdaGrad
// or FTRL context launches none of this file's instantiations.
//
// State row [2 (kp + 4)] = {m_V[kp], m_w, last, 0, 0, v_V[kp], v_w, 0, 0, 0}: the first and second moments (fp32) and,
// in the quad that carries m_w, the int32 step count `last` at which the row was last touched (its bits, stored by
// the quad's ordinary vector store; 0: never).  tau is the step being executed, counted from fm_create or the last
// fm_optimizer_reset (>= 1).  Per touched row, d = tau - last (1 for a row never touched), and per coordinate with
// g the run's fp64 gradient sum, gh = g / m, eta and lam StepParams' own:
//     m' = b1^d m + (1 - b1) gh          v' = b2^d v + (1 - b2) gh^2
//     x' = S_lam(v_cur - eta ((c1 m') / (sqrt(c2 v') + eps) + wd v_cur)),   c1 = 1 / (1 - b1^tau), c2 = 1 / (1 - b2^tau)
// in fp64, each stored word rounded once.  b^d is what dense Adam does to the moments of a coordinate whose
// gradient was zero for d - 1 steps; the parameter itself does not move in the gap (the lazy part).
//
// Registers.  Everything a coordinate needs besides its own words is uniform (kernel arguments: scalar registers)
// except the row's two decay factors, which the prologue computes once per lane per closing run as
// exp2(d log2 b) with log2 b from the host: two fp64 exp2 whose temporaries die before the coordinate loop, and
// four vector registers that live through it.  The walk never sees any of it.
#include <cmath>

#include "fm_window.h"

namespace fmhip {

namespace {

struct AdamRule {
  struct Hyper {
    double omb1, omb2;      // 1 - b1, 1 - b2
    double lg_b1, lg_b2;    // log2 b1, log2 b2
    double c1, c2;          // the step's bias factors 1 / (1 - b^tau)
    double eps, wd;
    int32_t tau;
  };
  struct Row {
    double b1d, b2d;  // b1^d, b2^d
  };
  using Args = WinArgs<AdamRule>;
  // quad = {m_w, last, 0, 0} as stored
  static __device__ __forceinline__ Row prologue(const Args& a, const float4& quad) {
    const int32_t last = __float_as_int(quad.y);
    const double d = last > 0 ? (double)(a.h.tau - last) : 1.0;
    return Row{exp2(d * a.h.lg_b1), exp2(d * a.h.lg_b2)};
  }
  static __device__ __forceinline__ float coord(float x, double g, float& m, float& v, const Args& a, const Row& r) {
    const double xd = (double)x, gh = g / a.p.m;
    const double mn = fma(r.b1d, (double)m, a.h.omb1 * gh);
    const double vn = fma(r.b2d, (double)v, a.h.omb2 * (gh * gh));
    m = (float)mn;
    v = (float)vn;
    const double step = a.p.eta * ((a.h.c1 * mn) / (sqrt(a.h.c2 * vn) + a.h.eps) + a.h.wd * xd);
    return (float)shrink_d(xd - step, a.p.lam);
  }
  static __device__ __forceinline__ float4 state_quad(float mw, const Args& a) {
    return make_float4(mw, __int_as_float(a.h.tau), 0.f, 0.f);
  }
};

}  // namespace

void launch_adam(const TableView& T, float* Z, int64_t N, const StepWork& w, FtrlWork& fw, const StepParams& p,
                 const AdamHyper& h, const uint32_t* skeys, const uint2* sents, int64_t n_loss_blocks, double* stats_out,
                 hipStream_t st) {
  AdamRule::Hyper hy;
  hy.omb1 = 1.0 - h.b1;
  hy.omb2 = 1.0 - h.b2;
  hy.lg_b1 = std::log2(h.b1);
  hy.lg_b2 = std::log2(h.b2);
  hy.c1 = 1.0 / (1.0 - std::pow(h.b1, (double)h.tau));
  hy.c2 = 1.0 / (1.0 - std::pow(h.b2, (double)h.tau));
  hy.eps = h.eps;
  hy.wd = h.wd;
  hy.tau = h.tau;
  launch_window_stage<AdamRule>(T, Z, N, w, fw, p, hy, skeys, sents, n_loss_blocks, stats_out, st);
}

}  // namespace fmhip
