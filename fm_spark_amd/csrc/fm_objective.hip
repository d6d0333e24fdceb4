// The objective stage of the single-table step (fm_config.loss != FM_LOSS_SQUARED): between the
// forward and the segmented update, k_objective replaces each sample's {r, yhat} pair by {r, r} with
// r the objective's derivative by that sample's score, and the forward's loss partials by its own.
//
// The seam.  The loss enters the update through those two fp32 words alone: the update forms
// t = x r, b = x^2 r and g_w = (x - 1) yh + r from them (fm_update.hip).  With yh := r its own
// expression gives g_w = x r, the true gradient of a loss whose derivative by the score is r, so no
// update kernel and no forward instantiation knows the objective.
//
// The score is the one the forward stored: yhat rounded to fp32 (the pair's second word).  That
// rounding is part of the contract (tests/objective_ref.py, round_scores=True).  Everything here is
// fp64 from that value on, in forms that stay finite for every finite score:
//   softplus(z) = max(z, 0) + log1p(exp(-|z|)),   sigma(z) = 1 / (1 + e) or e / (1 + e), e = exp(-|z|).
//
//   FM_LOSS_LOGISTIC  r_s = sigma(yhat_s) - y_s; a row with an entry adds softplus(yhat_s) - y_s yhat_s
//                     to the loss and 1 to the loss rows (the squared loss's rule).  One thread per row.
//   FM_LOSS_BPR       rows in groups of g: row p = q g the positive, the next g - 1 its negatives.
//                     d_j = yhat_p - yhat_{p+j}: r_{p+j} = sigma(-d_j), r_p = -sum_j sigma(-d_j), the
//                     loss sum_j softplus(-d_j), one loss row per (positive, negative) pair.  A team of
//                     TEAM lanes (1, 8 or 64 by g) owns a whole group: every lane reads the positive's
//                     score, lane l takes the negatives l + 1, l + 1 + TEAM, ... (each read and
//                     overwritten by that lane alone), the team's sums meet in an xor tree, and lane 0
//                     overwrites the positive's pair last -- behind the tree, which carries every lane's
//                     read of it.  So the stage works in place whatever the launch's block boundaries:
//                     no group is shared between teams.
//
// Every sum runs in a fixed order (a lane's rows ascending, the xor tree, block_loss_partial's waves
// in order; the update's combine folds the blocks' partials as it folds the forward's): equal inputs
// give equal bits.  No atomics.
#include "fm_device.h"

namespace fmhip {

namespace {

// blocks of the stage: one per CU; a larger batch strides the grid (<= kLossPartBlocks partials)
constexpr int kObjGrid = 256;
static_assert(kObjGrid <= kLossPartBlocks, "the stage's loss partials fit the reserved loss_part");

// (sigmoid_d / softplus_d: fm_device.h, shared with the binary evaluation)

template <int LOSS, int TEAM>
__global__ __launch_bounds__(kBlock) void k_objective(float2* __restrict__ yl, int64_t ystr,
                                                      const double* __restrict__ label,
                                                      const int64_t* __restrict__ row_ptr, int64_t n_rows, int32_t group,
                                                      double2* __restrict__ loss_part) {
  const int64_t gtid = (int64_t)blockIdx.x * kBlock + threadIdx.x, gthreads = (int64_t)gridDim.x * kBlock;
  double loss = 0.0, nloss = 0.0;
  if constexpr (LOSS == FM_LOSS_LOGISTIC) {
    for (int64_t s = gtid; s < n_rows; s += gthreads) {
      const double yh = (double)yl[s * ystr].y, y = label[s];
      const bool entries = row_ptr[s + 1] > row_ptr[s];
      const float r = (float)(sigmoid_d(yh) - y);
      yl[s * ystr] = make_float2(r, r);
      if (entries) {
        loss += softplus_d(yh) - y * yh;
        nloss += 1.0;
      }
    }
  } else {
    const int tl = threadIdx.x & (TEAM - 1);
    const int64_t g = group, n_groups = n_rows / g;
    for (int64_t q = gtid / TEAM; q < n_groups; q += gthreads / TEAM) {  // the same q on every lane of a team
      const int64_t p = q * g;
      const double yp = (double)yl[p * ystr].y;
      double sum = 0.0;
      for (int64_t j = 1 + tl; j < g; j += TEAM) {
        const double nd = (double)yl[(p + j) * ystr].y - yp;  // -d_j
        const double sg = sigmoid_d(nd);
        const float r = (float)sg;
        yl[(p + j) * ystr] = make_float2(r, r);
        sum += sg;
        loss += softplus_d(nd);
        nloss += 1.0;
      }
#pragma unroll
      for (int o = 1; o < TEAM; o <<= 1) sum += __shfl_xor(sum, o);
      if (tl == 0) {
        const float r = (float)(-sum);
        yl[p * ystr] = make_float2(r, r);
      }
    }
  }
  block_loss_partial(loss, nloss, loss_part);
}

template <int LOSS, int TEAM>
int64_t launch_obj(int64_t teams, const StepYl& v, const BatchDev& b, int32_t group, StepWork& w, hipStream_t st) {
  int64_t blocks = (teams * TEAM + kBlock - 1) / kBlock;
  if (blocks > kObjGrid) blocks = kObjGrid;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL((k_objective<LOSS, TEAM>), dim3((unsigned)blocks), dim3(kBlock), 0, st, v.yl, v.stride,
                     b.label.as<double>(), b.row_ptr.as<int64_t>(), b.n_rows, group, w.loss_part.as<double2>());
  FM_HIP_CHECK(hipGetLastError());
  return blocks;
}

}  // namespace

int64_t launch_objective(int32_t loss, int32_t group, int kp, const BatchDev& b, StepWork& w, hipStream_t st) {
  const StepYl v = step_yl(w, kp);
  w.loss_part.ensure(sizeof(double2) * kObjGrid);  // (reserve_work holds kLossPartBlocks: never grows here)
  if (loss == FM_LOSS_LOGISTIC) return launch_obj<FM_LOSS_LOGISTIC, 1>(b.n_rows, v, b, 0, w, st);
  FM_REQUIRE(loss == FM_LOSS_BPR, "unknown loss");
  FM_REQUIRE(group >= 2 && b.n_rows % group == 0, "the BPR objective needs whole groups of rows");
  const int64_t n_groups = b.n_rows / group;
  // a lane takes at most 4 (one thread per group), 8 or 16 negatives
  if (group <= 5) return launch_obj<FM_LOSS_BPR, 1>(n_groups, v, b, group, w, st);
  if (group <= 65) return launch_obj<FM_LOSS_BPR, 8>(n_groups, v, b, group, w, st);
  return launch_obj<FM_LOSS_BPR, 64>(n_groups, v, b, group, w, st);
}

}  // namespace fmhip
