"""GPU: the ranking calls against recorded bits (tests/golden/rank_bits.json).

tools/rank_bits.py runs small fixed problems through fm_rank_candidates / fm_rank_batch, their _select
forms and fm_rank_positions / fm_rank_positions_batch and digests the returned rows (or positions) and
scores; the fixture holds what a known-good build gave.  Unrestricted calls at C = 1023, 1025 and 2049,
n_top = 1 and 100, k = 4, 16 and 80; exclude lists that are empty, straddle a chunk edge and cover a
whole chunk; ragged ONLY lists with an empty one and one longer than a chunk; 600 contexts at
n_top = 1024, which the context tile cuts in two passes; positions with and without exclude lists, more
than 1,024 targets in one context and targets on their own exclude list; host rows and batches, finite
and infinite clamps -- over rows with absent ids, rows without a learned entry and rows equal in content.
(Whether the ranking is right is the question of tests/test_gpu_rank.py, test_gpu_rank_select.py and
test_gpu_rank_positions.py, against their references; this file only says when bits move.)  Equality is
exact.  The bits depend on the compiler too; see the tool's docstring for regenerating the fixture.
"""

import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import rank_bits  # noqa: E402

with open(os.path.join(ROOT, "tests", "golden", "rank_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_fixture_covers_every_case():
    assert sorted(GOLDEN) == sorted(rank_bits.CASES)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(rank_bits.CASES))
def test_rank_bits(gpu, name):
    assert rank_bits.run_case(name) == GOLDEN[name]
