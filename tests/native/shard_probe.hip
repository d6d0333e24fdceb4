// Test infrastructure (tests/shard_probe.py, tests/test_gpu_shard_phases.py), not part of the
// C-ABI: a thin extern "C" door to the sharded step's geometry seam of fm_shard.hip
// (fmhip::shard_geometry, fm_internal.h), so the suite can size batches against the tiles of the pair
// numbering, the trips of k_rows_scan, the grid-stride sweeps of k_sample_mask, k_route_keys,
// k_pair_table, k_shard_combine and k_pack_srec and the combine's team widths as the built library
// has them, not as a copy of its constants.  This file holds no kernel and launches none; it is
// compiled into the sort probe's library, beside the built libfm_hip.so it is linked against.  No
// exception crosses the boundary.
#include <exception>

#include "../../fm_spark_amd/csrc/fm_internal.h"

extern "C" {

// the geometry at the padded row width kp (a multiple of 4): out13 = {samples per pair tile, lanes per
// route team, samples per k_sample_mask sweep, tiles per k_rows_scan trip, entries per k_route_keys
// sweep, its unroll, entries per k_pair_table sweep, its unroll, kSlotRegs, kMaxR, the combine's
// team width at kp, its samples per sweep, the pairs per k_pack_srec sweep (0: no packed record)}
int shard_probe_geometry(int kp, int64_t* out13) {
  try {
    if (!out13 || kp < 4 || kp % 4) return FM_ERR_ARG;
    const fmhip::ShardGeometry g = fmhip::shard_geometry(kp);
    out13[0] = g.pair_tile;
    out13[1] = g.route_team;
    out13[2] = g.mask_sweep;
    out13[3] = g.scan_trip;
    out13[4] = g.route_sweep;
    out13[5] = g.route_unroll;
    out13[6] = g.table_sweep;
    out13[7] = g.table_unroll;
    out13[8] = g.slot_regs;
    out13[9] = g.max_r;
    out13[10] = g.combine_team;
    out13[11] = g.combine_sweep;
    out13[12] = g.pack_sweep;
    return FM_OK;
  } catch (const fmhip::Error& e) {
    return e.code;
  } catch (...) {
    return FM_ERR_HIP;
  }
}

}  // extern "C"
