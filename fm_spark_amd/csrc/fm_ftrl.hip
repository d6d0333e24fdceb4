// The FTRL-Proximal rule of the wave-per-window update stage (fm_window.h) for gfx950 (MI355X):
// fm_config.optimizer == FM_OPT_FTRL (McMahan et al., "Ad Click Prediction: a View from the Trenches", KDD 2013,
// algorithm 1).  The SGD and AdaGrad kernels are not touched, and a context of either launches none of these.
//
// Per touched coordinate, with g the run's fp64 gradient sum (fm_update.hip: g_V[f] = A[f] - v_cur[f] b,
// A = sum S (x r), b = sum x^2 r; g_w = sum (x - 1) yh + r), gh = g / m, alpha = stepSize, lambda1 = regParam,
// beta = opt_init, lambda2 = opt_l2, and the state words {z, n} (fp32):
//     if n == 0:  z = -v_cur (beta / alpha + lambda2) - sgn(v_cur) lambda1          (first touch)
//     n' = n + gh^2        z' = z + gh - ((sqrt(n') - sqrt(n)) / alpha) v_cur
//     v' = 0 if |z'| <= lambda1, else -(z' - sgn(z') lambda1) / ((beta + sqrt(n')) / alpha + lambda2)
// in fp64, each stored word rounded once (include/fm_hip.h has the reasons).  Nothing is ever pending on an FTRL
// context, whose cumulative shrink stands still.  The state row is [2 (kp + 4)] = {z_V, z_w, 0, 0, 0, n_V, n_w, 0, 0,
// 0}: the rule has no per-row scalars and its state quad leaves as {z_w, 0, 0, 0}.
//
// This file also holds what the stage's rules share on the host: the scratch's sizing, the state's zeroing and
// the suite's seams.
#include "fm_window.h"

namespace fmhip {

namespace {

__device__ __forceinline__ double sgn_d(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

struct FtrlRule {
  struct Hyper {
    double l1, beta, l2, inv_alpha;
  };
  struct Row {};
  using Args = WinArgs<FtrlRule>;
  static __device__ __forceinline__ Row prologue(const Args&, const float4&) { return Row{}; }
  // One coordinate: the state words advanced in place, the new value returned (fp64, each rounded once).
  static __device__ __forceinline__ float coord(float v, double g, float& z, float& n, const Args& a, const Row&) {
    const double vd = (double)v, nd = (double)n, gh = g * a.inv_m;
    double zd = (double)z;
    if (nd == 0.0) zd = -vd * (a.h.beta * a.h.inv_alpha + a.h.l2) - sgn_d(vd) * a.h.l1;  // first touch
    const double nn = nd + gh * gh;
    const double sn = sqrt(nn);
    const double zn = zd + gh - ((sn - sqrt(nd)) * a.h.inv_alpha) * vd;
    z = (float)zn;
    n = (float)nn;
    if (fabs(zn) <= a.h.l1) return 0.f;
    return (float)(-(zn - sgn_d(zn) * a.h.l1) / ((a.h.beta + sn) * a.h.inv_alpha + a.h.l2));
  }
  static __device__ __forceinline__ float4 state_quad(float zw, const Args&) { return make_float4(zw, 0.f, 0.f, 0.f); }
};

__global__ __launch_bounds__(kBlock) void k_ftrl_zero(float4* __restrict__ Z, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kBlock)
    Z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
}

int ftrl_stretch(int kp) { return kp <= 16 ? kFtrlWin / 16 : kFtrlWin / 4; }

}  // namespace

}  // namespace fmhip
// W in the low 16 bits, the stretch length of the kp <= 16 lane groups in the high 16
extern "C" int32_t fm_seam_ftrl_window(void) { return fmhip::kFtrlWin | (fmhip::ftrl_stretch(16) << 16); }
extern "C" int32_t fm_seam_ftrl_stretch(int32_t kp) { return fmhip::ftrl_stretch(kp); }
namespace fmhip {

void FtrlWork::ensure(int64_t N, int kp) {
  const size_t nwin = (size_t)std::max<int64_t>((N + kFtrlWin - 1) / kFtrlWin, 1);
  part.ensure_slack(sizeof(double) * 2 * nwin * (size_t)(kp + 2));
  ucnt.ensure_slack(sizeof(uint32_t) * ((nwin + kWavesPerBlock - 1) / kWavesPerBlock));
}

void launch_ftrl_zero(float* Z, int64_t rows, int kp, hipStream_t st) {
  if (rows <= 0) return;
  const int64_t n4 = rows * (2 * (kp + 4)) / 4;
  hipLaunchKernelGGL(k_ftrl_zero, dim3(grid_for(n4, kBlock)), dim3(kBlock), 0, st, reinterpret_cast<float4*>(Z), n4);
  FM_HIP_CHECK(hipGetLastError());
}

void launch_ftrl(const TableView& T, float* Z, int64_t N, const StepWork& w, FtrlWork& fw, const StepParams& p,
                 const FtrlHyper& h, const uint32_t* skeys, const uint2* sents, int64_t n_loss_blocks, double* stats_out,
                 hipStream_t st) {
  const FtrlRule::Hyper hy{h.l1, h.beta, h.l2, 1.0 / p.alpha};
  launch_window_stage<FtrlRule>(T, Z, N, w, fw, p, hy, skeys, sents, n_loss_blocks, stats_out, st);
}

}  // namespace fmhip
