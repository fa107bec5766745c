"""A plain `bench.py --gpus 1` run times the config-3 headline and nothing else, and --dump-outputs writes what the timed
path returned in its last step: the same AlignResult, bit for bit, as the same fixed-30 alignment made here."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_bench_line_and_dumped_outputs(gpu_lib, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out_dir = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"].startswith("NDT Gauss-Newton iters/sec") and line["unit"] == "iters/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["steps"] == 3 and line["warmup"] == 1 and line["value"] > 0 and line["ms_per_step"] > 0
    assert abs(line["value"] - 3 * 30 / (3 * line["ms_per_step"] * 1e-3)) < 0.01 * line["value"]
    for leg in ("batch", "3d", "cpu_baseline", "multi_start", "grid_build", "pose_err_vs_cpu_ref"):
        assert leg not in line                                    # --full only

    import torch
    from gtsam_ndt_amd import synth
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = synth.make_pair(3)
    tx, ty, sx, sy = (torch.from_numpy(d[k]).to("cuda:0") for k in ("tx", "ty", "sx", "sy"))
    torch.cuda.synchronize()
    with NdtMatcher2D(device=0, fixed_iterations=30) as m:
        m.set_target(tx, ty)
        m.align_async(sx, sy, d["init"], producer_complete=True)
        r = m.finish()
    want = {"pose": r.pose, "H": r.H, "g": r.g, "score": [r.score], "iterations": [r.iterations], "n_hit": [r.n_hit],
            "status": [r.status]}
    assert sorted(os.listdir(out_dir)) == sorted(f"{k}.npy" for k in want)
    for k, v in want.items():
        got = np.load(out_dir / f"{k}.npy")
        assert got.dtype == np.float64
        np.testing.assert_array_equal(got, np.asarray(v, dtype=np.float64))
    assert r.iterations == 30 and r.status == 0
