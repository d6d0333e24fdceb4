"""GPU: the step's update paths against recorded bits (tests/golden/step_bits.json).

tools/step_bits.py runs small fixed problems through fm_step_batch (and fm_repl_grad /
fm_repl_apply) and digests the loss history and the exported tables; the fixture holds what a
known-good build gave.  Fused and unfused steps, prepared and unprepared batches, k = 3 .. 80,
with absent rows, empty rows, a row long enough for the fused forward's overflow walk and runs of
2, 300 and 768 entries, three steps with regParam > 0.  (Whether the update's pieces and combines are
right at their group, wave, block and range edges is tests/test_gpu_update_edges.py's question, against
the oracle; this file only says when bits move.)  The sharded cases run the same problems through a sharded context of
R = 1 .. 12 ranks on one device, both wires, and add the digest of fm_predict on the trained tables:
every team width and both owner-access variants of the requester's combine, and its predict with
absent rows counted.  Equality is exact: a change to the forward, the segmented update, its
combine, the replicated apply, or the sharded combine and predict that moves one bit of a table, a
loss or a prediction shows here.  The bits
depend on the compiler too; see the tool's docstring for regenerating the fixture.
"""

import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import step_bits  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "step_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_every_case():
    assert sorted(GOLDEN) == sorted(step_bits.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(step_bits.CASES))
def test_step_bits(gpu, name):
    got = step_bits.run_case(name)
    assert got["loss"] == GOLDEN[name]["loss"]
    assert got["tables"] == GOLDEN[name]["tables"]
    assert got.get("predict") == GOLDEN[name].get("predict")
