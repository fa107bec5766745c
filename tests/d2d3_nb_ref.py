"""float64 restatement of the map neighbourhood of 3D map-to-map alignment, docs/ALGORITHM.md §2.26: a source component
is scored against the target voxel its mean falls into and that voxel's six face neighbours.

TEST INFRASTRUCTURE ONLY (imported by tests/test_d2d3_nb_ref.py and tests/test_gpu_d2d3_neighbourhood.py).  Built on
tests/d2d3_ref.py without a line of its own arithmetic: the objective is a sum over component-voxel pairs, so the sums
of neighbourhood 7 are d2d3_ref.evaluate's sums once per candidate, each time with the candidate's voxel in the place
of the component's own.  The one thing that changes per candidate is the lookup, and d2d3_ref.evaluate takes its pairs
from the module's `lookup`; `_candidate` puts the candidate's (key, hit, image) there for the duration of one call.
"""
from __future__ import annotations

import contextlib

import numpy as np

import d2d3_ref as R
from oracle import ndt3d as O

# §2.25's candidate order: own, x-1, x+1, y-1, y+1, z-1, z+1
OFFSETS = ((0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
EVAL_FLOOR = R.EVAL_FLOOR


def candidates(tgt: O.Grid3D, comps: R.Components3, pose, nb: int):
    """[(key int64 [n], hit bool [n])] per candidate, and the float32 images.  The own voxel is d2d3_ref.lookup's; a
    neighbour is taken by INDEX: one that leaves [0, W) x [0, H) x [0, D) is skipped (key 0, no hit), and a component
    whose own image is outside the grid has no candidate at all."""
    assert nb in (1, 7)
    W, H, D = (int(v) for v in tgt.dims)
    key, _, P = R.lookup(tgt, comps, pose)
    _, inside = O.cell_keys3(P, tgt.o, tgt.inv_c, tgt.dims)
    ix, iy, iz = key % W, (key // W) % H, key // (W * H)
    out = []
    for dx, dy, dz in OFFSETS[:nb]:
        jx, jy, jz = ix + dx, iy + dy, iz + dz
        ok = inside & (jx >= 0) & (jx < W) & (jy >= 0) & (jy < H) & (jz >= 0) & (jz < D)
        k = np.where(ok, (jz * H + jy) * W + jx, 0)
        out.append((k, ok & tgt.valid[k]))
    return out, P


@contextlib.contextmanager
def _candidate(key, hit, P):
    own = R.lookup
    R.lookup = lambda tgt, comps, pose: (key, hit, P)
    try:
        yield
    finally:
        R.lookup = own


def evaluate_nb(tgt: O.Grid3D, comps: R.Components3, pose, prm: O.Ndt3Params, nb: int, mirror32: bool = False):
    """H (6x6), g (6), score, n_hit over the candidates, added in candidate order; n_hit counts component-voxel pairs."""
    pose = tuple(float(v) for v in pose)
    cands, P = candidates(tgt, comps, pose, nb)
    H, g, sc, n_hit = np.zeros((6, 6)), np.zeros(6), 0.0, 0
    for key, hit in cands:
        with _candidate(key, hit, P):
            Hc, gc, sc_c, nc = R.evaluate(tgt, comps, pose, prm, mirror32)
        H, g, sc, n_hit = H + Hc, g + gc, sc + sc_c, n_hit + nc
    return H, g, sc, n_hit


def align_nb(tgt: O.Grid3D, comps: R.Components3, init_pose, prm: O.Ndt3Params, nb: int, mirror32: bool = False):
    """d2d3_ref.align's loop (oracle.ndt3d.gn_update3) over evaluate_nb."""
    pose = tuple(float(v) for v in init_pose)
    it = 0
    if comps.n < 1 or tgt.n_valid < 1:
        return {"pose": pose, "H": np.zeros((6, 6)), "g": np.zeros(6), "score": 0.0, "n_hit": 0, "iterations": 0,
                "status": O.NDT_TOO_FEW_CELLS}
    ls = {} if prm.line_search > 0 else None
    while True:
        H, g, sc, n_hit = evaluate_nb(tgt, comps, pose, prm, nb, mirror32)
        pose, it, status, done = O.gn_update3(pose, H, g, n_hit, it, prm, sc, ls)
        if done:
            return {"pose": pose, "H": H, "g": g, "score": sc, "n_hit": n_hit, "iterations": it, "status": status}


def n_border(tgt: O.Grid3D, comps: R.Components3, pose) -> int:
    """Components whose f = (p' - o) inv_c lies within 4 float32 ulps of an integer on some axis: the ones whose own
    voxel another rounding of the image could flip."""
    _, _, P = R.lookup(tgt, comps, tuple(float(v) for v in pose))
    f = (P.astype(np.float32) - tgt.o.astype(np.float32)) * np.float32(tgt.inv_c)
    ulp = np.spacing(np.maximum(np.abs(f), np.float32(1.0)).astype(np.float32))
    near = np.abs(f.astype(np.float64) - np.rint(f.astype(np.float64))) <= 4.0 * ulp.astype(np.float64)
    return int(np.count_nonzero(np.any(near, axis=1)))


def eval_bounds_nb(cases, prm: O.Ndt3Params, nb: int = 7):
    """d2d3_ref.eval_bounds' recipe over evaluate_nb: 4 x the largest mirror32-vs-float64 eval_diffs over
    `cases` = [(tgt, comps, pose)], floored at EVAL_FLOOR.  Returns (bounds [3], measured [3])."""
    gn = O.Ndt3Params(**{**prm.__dict__, "hessian_mode": 0})
    worst = np.zeros(3)
    for tgt, comps, pose in cases:
        Hgn = evaluate_nb(tgt, comps, pose, gn, nb)[0]
        d = R.eval_diffs(evaluate_nb(tgt, comps, pose, prm, nb, mirror32=True), evaluate_nb(tgt, comps, pose, prm, nb), Hgn)
        worst = np.maximum(worst, d)
    return np.maximum(4.0 * worst, EVAL_FLOOR), worst


def build_map_at(o, dims, x, y, z, prm: O.Ndt3Params):
    """(grid, components) of a point set in a grid whose geometry is GIVEN (origin o, extents dims), as a reserved
    target's is: oracle.ndt3d.build_grid3's sums and records without its guard ring, so that voxels at index 0 and at
    W - 1 can be occupied.  Every point has to lie inside."""
    P32 = np.stack([np.asarray(x, np.float32), np.asarray(y, np.float32), np.asarray(z, np.float32)], axis=1)
    o = np.asarray(o, np.float32)
    inv_c = np.float32(1.0 / float(prm.cell_size))
    dims = tuple(int(v) for v in dims)
    key, inside = O.cell_keys3(P32, o, inv_c, dims)
    assert inside.all()
    nc = dims[0] * dims[1] * dims[2]
    P = P32.astype(np.float64)
    count = np.bincount(key, minlength=nc).astype(np.int64)
    nz = np.maximum(count, 1)[:, None]
    mean = np.stack([np.bincount(key, weights=P[:, a], minlength=nc) for a in range(3)], axis=1) / nz
    d = P - mean[key]
    mean = mean + np.stack([np.bincount(key, weights=d[:, a], minlength=nc) for a in range(3)], axis=1) / nz
    d = P - mean[key]
    M2 = np.stack([np.bincount(key, weights=d[:, i] * d[:, j], minlength=nc) for i, j in R.SYM], axis=1)
    cand = np.nonzero(count >= max(prm.min_points, 2))[0]
    valid = np.zeros(nc, bool)
    icov = np.zeros((nc, 6))
    if cand.size:
        ok, ic = O.finalise_cells3(count[cand], M2[cand], prm)
        valid[cand] = ok
        icov[cand] = ic
    mean[~valid] = 0.0
    g = O.Grid3D(o, inv_c, dims, count, mean, icov, valid, int(valid.sum()))
    return g, R.components(g)


# The hand-built grid of the edge tests: 6 x 5 x 4 voxels of 1 m from the origin, six occupied voxels on its faces in
# three pairs that key arithmetic alone would take for neighbours: keys 1 apart across a row's end, keys W apart across
# a layer's end, and the two ends of a column (key -/+ W H from there is no voxel at all).
EDGE_DIMS = (6, 5, 4)
EDGE_VOXELS = ((5, 1, 1), (0, 2, 1), (2, 4, 1), (2, 0, 2), (3, 2, 0), (3, 2, 3))


def voxel_points(v, seed=5, n=16):
    """n points scattered over voxel v (index triple) of a 1 m grid at the origin; they depend on seed and voxel alone."""
    return (np.array(v) + 0.5 + np.random.default_rng([seed, *v]).uniform(-0.45, 0.45, size=(n, 3))).astype(np.float32)


def pose_error(p, q):
    """(translation norm, rotation-parameter norm) of p - q."""
    p, q = np.asarray(p, dtype=np.float64), np.asarray(q, dtype=np.float64)
    return float(np.linalg.norm(p[:3] - q[:3])), float(np.linalg.norm(p[3:] - q[3:]))
