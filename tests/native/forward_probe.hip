// Test infrastructure (tests/forward_probe.py, tests/test_gpu_forward_teams.py), not part of the
// C-ABI: a thin extern "C" door to the forward's launch-size seam of fm_forward.hip
// (fmhip::set_forward_grid_cap and the launch log, fm_internal.h), so the suite can make every team
// of k_forward walk several samples at a batch of a few hundred rows and assert on what was
// launched.  This file holds no kernel and launches none; it is compiled into the sort probe's
// library, beside the built libfm_hip.so it is linked against.  No exception crosses the boundary.
#include <exception>

#include "../../fm_spark_amd/csrc/fm_internal.h"

namespace {

template <class F>
int guarded(F&& f) {
  try {
    return f();
  } catch (const fmhip::Error& e) {
    return e.code;
  } catch (...) {
    return FM_ERR_HIP;
  }
}

}  // namespace

extern "C" {

// the layout tests/forward_probe.py reads (int64 words)
struct fwd_probe_rec {
  int64_t mode, gs, team, u, chunk, chunks, blocks, rows;
};

// blocks > 0: every forward launch of the process takes at most that many blocks and is logged;
// 0: the tuned grid, nothing logged
int fwd_probe_set_grid_cap(int64_t blocks) {
  return guarded([&]() -> int {
    FM_REQUIRE(blocks >= 0, "negative grid cap");
    fmhip::set_forward_grid_cap(blocks);
    return FM_OK;
  });
}

int fwd_probe_clear_log(void) {
  return guarded([&]() -> int {
    fmhip::clear_forward_log();
    return FM_OK;
  });
}

// out[cap] receives the first records; *n_logged = the launches made under a cap since the last clear
// (more than the records kept when the log's bound was reached); returns the number of records written
int fwd_probe_read_log(fwd_probe_rec* out, int cap, int64_t* n_logged) {
  int written = 0;
  const int st = guarded([&]() -> int {
    FM_REQUIRE(out && n_logged && cap >= 0, "null argument");
    fmhip::FwdLaunchRec recs[fmhip::kFwdLogCap];
    const int total = fmhip::read_forward_log(recs, fmhip::kFwdLogCap);
    const int have = total < fmhip::kFwdLogCap ? total : fmhip::kFwdLogCap;
    for (; written < have && written < cap; ++written) {
      const fmhip::FwdLaunchRec& r = recs[written];
      out[written] = fwd_probe_rec{r.mode, r.gs, r.team, r.u, r.chunk, r.chunks, r.blocks, r.rows};
    }
    *n_logged = total;
    return FM_OK;
  });
  return st == FM_OK ? written : st;  // statuses are negative
}

// the forward's constants a test needs: {tuned block cap, threads per block, kFuseNS, kFuseU, log bound}
int fwd_probe_consts(int64_t* out5) {
  return guarded([&]() -> int {
    FM_REQUIRE(out5, "null argument");
    const fmhip::FwdConsts c = fmhip::forward_consts();
    out5[0] = c.grid;
    out5[1] = c.block;
    out5[2] = c.fuse_ns;
    out5[3] = c.fuse_u;
    out5[4] = fmhip::kFwdLogCap;
    return FM_OK;
  });
}

}  // extern "C"
