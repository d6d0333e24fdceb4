// Test infrastructure (tests/update_probe.py, tests/test_gpu_update_edges.py), not part of the
// C-ABI: a thin extern "C" door to the update side's geometry seam of fm_update.hip
// (fmhip::update_geometry, fm_internal.h), so the suite can place runs of equal keys against the
// groups, waves and blocks of k_segment_update, the ranges of k_segment_combine and the chunks of
// k_split_* as the built library has them, not as a copy of its constants.  This file holds no
// kernel and launches none; it is compiled into the sort probe's library, beside the built
// libfm_hip.so it is linked against.  No exception crosses the boundary.
#include <exception>

#include "../../fm_spark_amd/csrc/fm_internal.h"

extern "C" {

// the geometry at the padded row width kp (a multiple of 4, as a context's TableView has it):
// out8 = {entries per wave, per group, per block, paired stores, combine lanes per range,
// kCombCols, split chunk, scan chunks per round}
int upd_probe_geometry(int kp, int64_t* out8) {
  try {
    if (!out8 || kp < 4 || kp % 4) return FM_ERR_ARG;
    const fmhip::UpdGeometry g = fmhip::update_geometry(kp);
    out8[0] = g.wave_entries;
    out8[1] = g.group_entries;
    out8[2] = g.block_entries;
    out8[3] = g.paired;
    out8[4] = g.comb_lanes;
    out8[5] = g.comb_cols;
    out8[6] = g.split_chunk;
    out8[7] = g.scan_round_chunks;
    return FM_OK;
  } catch (const fmhip::Error& e) {
    return e.code;
  } catch (...) {
    return FM_ERR_HIP;
  }
}

}  // extern "C"
