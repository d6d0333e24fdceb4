// Stand-alone host check (tests/test_host_sanitizers.py, AddressSanitizer on the host code): a
// multi-GPU batch may outlive its context (include/fm_hip.h, fm_batch_destroy).  GroupBatch::g points
// at the group only while the batch is the group's pending prepare; a batch that was prepared and
// finished, or replaced, and is destroyed after the group must not touch the freed group.  The group
// and batches here have no ranks and no parts, so no device call is made.
#include "../../fm_spark_amd/csrc/fm_group.hip"
#include <cstdio>
int main() {
  using namespace fmhip;
  {  // prepared and finished (drop_route's path), then context first
    Group* g = new Group();
    GroupBatch* gb = new GroupBatch();
    g->set_pending(*gb);
    gb->routed = true;
    drop_route(*g, *gb);
    if (gb->g != nullptr || g->pending != nullptr) { printf("link not cleared\n"); return 1; }
    delete g;
    delete gb;
  }
  {  // still pending when the group goes
    Group* g = new Group();
    GroupBatch* gb = new GroupBatch();
    g->set_pending(*gb);
    delete g;
    if (gb->g != nullptr) { printf("stale g\n"); return 1; }
    delete gb;
  }
  {  // two batches prepared in turn; the first is destroyed after the group
    Group* g = new Group();
    GroupBatch* a = new GroupBatch();
    GroupBatch* b = new GroupBatch();
    g->set_pending(*a);
    g->set_pending(*b);
    if (a->g != nullptr) { printf("stale g on the replaced batch\n"); return 1; }
    delete b;
    if (g->pending != nullptr) { printf("pending not cleared\n"); return 1; }
    delete g;
    delete a;
  }
  printf("0 failure(s)\n");
  return 0;
}
