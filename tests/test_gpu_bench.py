"""GPU: bench.py's launch paths measure the same training.

The single-table step (fused and unfused), the one-process multi-GPU group context on one GPU
(--force-sharded: the row-sharded protocol with RCCL and one rank, what INTEGRATION.md's
createMulti gives a Spark driver) and its replicated layout must train the same model: the sum of
every executed step's loss agrees to 1e-6 (different but fixed summation orders).  Asking for more
GPUs than the box has must exit non-zero without a JSON line (no silent downgrade to one rank).
These read the line's kernel phases and host trace, so they run the benchmark with --full.  A plain
run times its steps and nothing else, and --dump-outputs writes the same arrays from run to run.
"""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = ["--features", "200000", "--rows", "16384", "--steps", "6", "--warmup", "2", "--batches", "2"]
SMALL = [*SHAPE, "--full", "--no-cpu-baseline", "--host-path-steps", "0"]


def _bench(*extra, check=True, base=SMALL):
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *base, *extra], capture_output=True,
                       text=True, timeout=100, env=env, cwd=ROOT)
    if not check:
        return p
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def single(gpu):
    return _bench("--fuse", "off")


def test_fused_single_table_trains_the_same_model(single):
    fused = _bench("--fuse", "on")
    assert "split" in fused["kernels"] and "split" not in single["kernels"]
    assert fused["loss_sum_all_steps"] == pytest.approx(single["loss_sum_all_steps"], rel=1e-6)


def test_group_path_on_one_gpu_matches_single_table(single):
    g = _bench("--force-sharded")
    assert g["config"]["launch"] == "group" and g["n_gpus"] == 1
    assert "owner_update" in g["kernels"]
    assert g["loss_sum_all_steps"] == pytest.approx(single["loss_sum_all_steps"], rel=1e-6)
    assert g["host_trace"]["step_enqueue_ms_median"] < g["ms_per_step"]


def test_replicated_group_on_one_gpu_matches_single_table(single):
    r = _bench("--parallel", "replicated")
    assert r["config"]["launch"] == "group" and "replicated" in r["config"]["parallelism"]
    assert r["loss_sum_all_steps"] == pytest.approx(single["loss_sum_all_steps"], rel=1e-6)


def test_more_gpus_than_visible_exits_nonzero(gpu):
    import torch

    n = torch.cuda.device_count()
    p = _bench("--gpus", str(n + 1), check=False)
    assert p.returncode != 0
    assert f"needs {n + 1} visible GPUs" in p.stderr and '"metric"' not in p.stdout


def test_plain_run_times_its_steps_only_and_dumps_the_same_outputs(single, tmp_path):
    """Without --full the line carries the headline and none of the legs; --dump-outputs writes the
    loss history and a fixed sample of the model's rows in float64, under 64 MB, the same from run to
    run (same ids; the values to fp32 rounding of fixed-order sums), and the same training as --full."""
    import numpy as np

    runs = []
    for d in ("a", "b"):
        line = _bench("--fuse", "off", "--dump-outputs", str(tmp_path / d), base=SHAPE)
        assert line["steps"] == 6 and line["warmup"] == 2 and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(16384 / (line["ms_per_step"] * 1e-3), rel=1e-9)
        for leg in ("kernels", "roofline", "step_roofline", "host_path", "fit", "cpu_baseline"):
            assert leg not in line, leg
        out = {f[:-4]: np.load(tmp_path / d / f) for f in sorted(os.listdir(tmp_path / d))}
        assert sorted(out) == ["V", "ids", "loss_history", "present", "w"]
        assert all(a.dtype == np.float64 for a in out.values())
        assert sum(a.nbytes for a in out.values()) <= 64 << 20
        n = len(out["ids"])
        assert out["w"].shape == (n,) and out["V"].shape == (n, 16) and out["present"].all()
        assert len(out["loss_history"]) == 8  # warmup + timed steps
        assert float(out["loss_history"].sum()) == pytest.approx(line["loss_sum_all_steps"], rel=1e-12)
        assert line["loss_sum_all_steps"] == pytest.approx(single["loss_sum_all_steps"], rel=1e-6)
        assert np.abs(out["V"]).max() > 0 and np.isfinite(out["V"]).all()
        runs.append(out)
    a, b = runs
    np.testing.assert_array_equal(a["ids"], b["ids"])
    for name in ("loss_history", "w", "V"):
        np.testing.assert_allclose(a[name], b[name], rtol=1e-6, atol=1e-9)
