"""Float64 restatement of the score of a pose list (docs/ALGORITHM.md "Scoring a list of poses"): what
ndt2d_score_poses* / ndt3d_score_poses* are held to.  The transform and the cell keys mirror the device's float32
arithmetic (the oracle's mirror32); the terms and the sums are float64.

2D follows _oracle_volume of test_gpu_search.py, with one (x, y, theta) per row instead of a lattice; 3D calls
oracle.ndt3d.evaluate3(mirror32=True) per pose.  A pose with a non-finite coordinate scores 0; NaN points of the scan
add nothing."""
import math

import numpy as np


def scores2d(grids, sx, sy, poses, prm):
    """scores [m] (float64) of the scan at poses [m, 3] against the oracle's grid or list of grids (overlap_grids)."""
    from oracle import ndt2d as o
    if not isinstance(grids, (list, tuple)):
        grids = [grids]
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    ok = np.isfinite(sx) & np.isfinite(sy)
    x, y = np.asarray(sx)[ok].astype(np.float32), np.asarray(sy)[ok].astype(np.float32)
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    out = np.zeros(poses.shape[0])
    for i, (tx, ty, t) in enumerate(poses):
        if not (math.isfinite(tx) and math.isfinite(ty) and math.isfinite(t)):
            continue
        c32, s32 = np.float32(math.cos(t)), np.float32(math.sin(t))
        tx32, ty32 = np.float64(np.float32(tx)), np.float64(np.float32(ty))
        # px = fmaf(c, x, fmaf(-s, y, tx));  py = fmaf(s, x, fmaf(c, y, ty))
        inner_x = (y64 * np.float64(-s32) + tx32).astype(np.float32)
        inner_y = (y64 * np.float64(c32) + ty32).astype(np.float32)
        px = (x64 * np.float64(c32) + inner_x.astype(np.float64)).astype(np.float32)
        py = (x64 * np.float64(s32) + inner_y.astype(np.float64)).astype(np.float32)
        for g in grids:
            key, inside = o.cell_keys32(px, py, g.ox, g.oy, g.inv_c, g.W, g.H)
            hit = inside & g.valid[key]
            qx = px.astype(np.float64) - g.mean[key, 0]
            qy = py.astype(np.float64) - g.mean[key, 1]
            a, b, cc = g.icov[key, 0], g.icov[key, 1], g.icov[key, 2]
            mm = qx * (a * qx + b * qy) + qy * (b * qx + cc * qy)
            with np.errstate(over="ignore", invalid="ignore"):
                s = np.where(hit, prm.d1 * np.exp(-0.5 * prm.d2 * np.where(hit, mm, 0.0)), 0.0)
            out[i] += s.sum()
    return out


def scores3d(grid, sx, sy, sz, poses, prm):
    """scores [m] (float64) of the scan at poses [m, 6] against the oracle's voxel grid."""
    from oracle import ndt3d as o
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 6)
    ok = np.isfinite(sx) & np.isfinite(sy) & np.isfinite(sz)
    x, y, z = (np.asarray(a)[ok] for a in (sx, sy, sz))
    out = np.zeros(poses.shape[0])
    for i, p in enumerate(poses):
        if np.all(np.isfinite(p)):
            out[i] = o.evaluate3(grid, x, y, z, tuple(float(v) for v in p), prm, mirror32=True)[2]
    return out
