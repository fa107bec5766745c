"""The float64 restatement of the pose-list score (tests/score_poses_ref.py) against the oracles' single-pose
evaluation, on the CPU: the GPU tests hold ndt2d/ndt3d_score_poses* to it.  These tests check the yardstick against
the oracle and call nothing of the library, so, unlike the other new test files, they pass without the new entry points."""
import math
import os

import numpy as np
import pytest

import score_poses_ref as R
from gtsam_ndt_amd import synth

GOLD3 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ndt3d_small.npz")


@pytest.mark.parametrize("overlap", [1, 4])
def test_the_2d_restatement_is_the_oracles_evaluation(overlap):
    """Both mirror the float32 transform and keys.  The oracle's mirror32 evaluation also rounds the cell records to
    float32, the restatement (as _oracle_volume of test_gpu_search.py) keeps them in float64: a mean moves by at most
    2^-24 |mean| < 6e-7 m here (|mean| < 10 m), which with |Sigma^-1 q| up to 1e3 /m moves the exponent by about 1e-3
    at worst, and so a term by that fraction: 2e-3 relative, far below what a wrong key or a wrong pose would show."""
    from oracle import ndt2d as o
    d = synth.make_pair(1)
    prm = o.NdtParams(overlap=overlap)
    grids = o.build_grids(d["tx"], d["ty"], prm)
    c = d["init"]
    poses = np.array([c, (c[0] + 0.3, c[1] - 0.2, c[2] + 0.4), (c[0] - 0.7, c[1] + 0.5, c[2] + 2.0 * math.pi + 0.1),
                      (c[0], c[1], c[2] - 3.0), (40.0, 40.0, 0.0)])
    got = R.scores2d(grids, d["sx"], d["sy"], poses, prm)
    want = np.array([o.evaluate(grids, d["sx"], d["sy"], tuple(p), prm, mirror32=True)[2] for p in poses])
    print(got, want)
    assert np.all(np.abs(got - want) <= 2e-3 * np.abs(want))
    assert want[0] > 10.0 and want[-1] == 0.0 and got[-1] == 0.0


def test_the_2d_restatement_skips_nan_points_and_zeroes_non_finite_poses():
    from oracle import ndt2d as o
    d = synth.make_pair(1)
    prm = o.NdtParams()
    g = o.build_grid(d["tx"], d["ty"], prm)
    sx, sy = d["sx"].copy(), d["sy"].copy()
    base = R.scores2d(g, sx[10:], sy[10:], [d["init"]], prm)
    sx[:5] = np.nan
    sy[5:10] = np.nan
    poses = [d["init"], (math.nan, 0.0, 0.0), (0.0, math.inf, 0.0), (0.0, 0.0, -math.inf)]
    got = R.scores2d(g, sx, sy, poses, prm)
    assert got[0] == base[0] and np.all(got[1:] == 0.0)


def test_the_3d_restatement_is_the_oracles_evaluation():
    from oracle import ndt3d as o
    z = np.load(GOLD3)
    t = [np.ascontiguousarray(z[k], dtype=np.float32) for k in ("tx", "ty", "tz")]
    s = [np.ascontiguousarray(z[k], dtype=np.float32)[:1024] for k in ("sx", "sy", "sz")]
    p = tuple(float(v) for v in z["final_pose"])
    prm = o.Ndt3Params()
    g = o.build_grid3(*t, prm)
    poses = [p, (p[0] + 0.2, p[1], p[2] - 0.1, p[3] + 0.03, p[4], p[5] + 0.2), (math.nan,) + p[1:], p[:4] + (math.inf, p[5])]
    s_nan = [np.concatenate([a, [np.nan]]).astype(np.float32) for a in s]
    got = R.scores3d(g, *s_nan, poses, prm)
    want = [o.evaluate3(g, *s, q, prm, mirror32=True)[2] for q in poses[:2]]
    assert got[0] == want[0] and got[1] == want[1] and got[0] > got[1] > 0.0
    assert got[2] == 0.0 and got[3] == 0.0
