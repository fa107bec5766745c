"""float64 restatement of 2D map-to-map alignment (distribution-to-distribution NDT), docs/ALGORITHM.md §2.13.

TEST INFRASTRUCTURE ONLY (imported by tests/test_d2d_ref.py and tests/test_gpu_d2d.py): built on
oracle.ndt2d.build_grid for both maps and on oracle.ndt2d.gn_update for the step, so everything but the
per-component terms is the code the point-to-map tests already trust.

A *component* is a valid cell of a grid: its mean and its regularised covariance, the float64 inverse of the
`icov` the oracle stores.  The source map is its component list in cell-key order, the target map is looked up
by the single-cell source-side rule of §2.1 at the float32 image of the component's mean (the contract's key:
float32 records, image_point's fmaf order), in both modes below, so the two modes see the same pairs:
  mirror32=False  the truth: float64 means and covariances, float64 arithmetic
  mirror32=True   the float32 records and every per-component operation rounded to float32 (the order the
                  kernel uses, without its fma contraction), summed in float64; what the GPU tests take their
                  bound from
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from oracle import ndt2d as O


@dataclass
class Components:
    key: np.ndarray     # int64 [n]   cell keys, ascending
    mean: np.ndarray    # float64 [n, 2]
    cov: np.ndarray     # float64 [n, 3]  (xx, xy, yy) of the regularised covariance

    @property
    def n(self) -> int:
        return int(self.key.shape[0])


def cov_from_icov(icov: np.ndarray) -> np.ndarray:
    """(a, b, c) of Sigma^-1 -> (xx, xy, yy) of Sigma, float64; rows of zeros stay zeros."""
    a, b, c = icov[:, 0], icov[:, 1], icov[:, 2]
    det = a * c - b * b
    ok = det > 0.0
    r = np.where(ok, 1.0 / np.where(ok, det, 1.0), 0.0)
    return np.stack([c * r, -b * r, a * r], axis=1)


def components(grid: O.Grid2D) -> Components:
    k = np.nonzero(grid.valid)[0].astype(np.int64)          # ascending = cell-key order
    return Components(k, grid.mean[k].copy(), cov_from_icov(grid.icov[k]))


def build_map(x, y, prm: O.NdtParams, bounds=None):
    """(grid, components) of a point set: what a handle holds after set_target / add_target_points."""
    g = O.build_grid(x, y, prm, bounds=bounds)
    return g, components(g)


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def lookup(tgt: O.Grid2D, comps: Components, pose):
    """Target cell of every source component at `pose` by the contract's float32 rule.  Returns
    (key int64 [n], hit bool [n], px, py float32 [n]): the clamped-key lookup of the kernels lands every
    outside image on an (invalid) ring cell, which the inside test of cell_keys32 restates."""
    tx, ty, th = (float(v) for v in pose)
    c32, s32 = np.float32(math.cos(th)), np.float32(math.sin(th))
    mx, my = _f32(comps.mean[:, 0]), _f32(comps.mean[:, 1])
    px = O._fma32(mx, c32, O._fma32(my, -s32, np.float32(tx)))
    py = O._fma32(mx, s32, O._fma32(my, c32, np.float32(ty)))
    key, inside = O.cell_keys32(px, py, tgt.ox, tgt.oy, tgt.inv_c, tgt.W, tgt.H)
    hit = inside & tgt.valid[key]
    return key, hit, px, py


def evaluate(tgt: O.Grid2D, comps: Components, pose, prm: O.NdtParams, mirror32: bool = False, pairs: list | None = None):
    """H (3x3), g (3), score, n_hit of f = -sum_i d1 exp(-d2/2 q' (R S_i R' + S_j)^-1 q) at `pose`.
    pairs (optional list): receives the array of target keys per component (-1: no hit)."""
    tx, ty, th = (float(v) for v in pose)
    key, hit, px32, py32 = lookup(tgt, comps, pose)
    if pairs is not None:
        pairs.append(np.where(hit, key, -1))
    k = key[hit]
    tcov = cov_from_icov(tgt.icov[k])
    if mirror32:
        F = np.float32
        cs, sn = F(math.cos(th)), F(math.sin(th))
        t_x, t_y = F(tx), F(ty)
        px, py = px32[hit], py32[hit]
        sa, sb, sc = (_f32(comps.cov[hit, j]) for j in range(3))
        mean32 = tgt.records32()[0]
        mjx, mjy = mean32[k, 0], mean32[k, 1]
        ta, tb, tc = (_f32(tcov[:, j]) for j in range(3))
        d1, d2 = F(prm.d1), F(prm.d2)
        c2t, s2t = cs * cs - sn * sn, F(2.0) * cs * sn
    else:
        F = np.float64
        cs, sn = math.cos(th), math.sin(th)
        t_x, t_y = tx, ty
        mx, my = comps.mean[hit, 0], comps.mean[hit, 1]
        px = cs * mx - sn * my + tx
        py = sn * mx + cs * my + ty
        sa, sb, sc = (comps.cov[hit, j] for j in range(3))
        mjx, mjy = tgt.mean[k, 0], tgt.mean[k, 1]
        ta, tb, tc = (tcov[:, j] for j in range(3))
        d1, d2 = prm.d1, prm.d2
        c2t, s2t = cs * cs - sn * sn, 2.0 * cs * sn
    half, two = F(0.5), F(2.0)
    # S = R Sigma_i R' through the half trace / half difference: Sxx = hm + u, Syy = hm - u
    hm, hd = half * (sa + sc), half * (sa - sc)
    u = hd * c2t - sb * s2t
    sxy = hd * s2t + sb * c2t
    axx, axy, ayy = (hm + u) + ta, sxy + tb, (hm - u) + tc
    rdet = F(1.0) / (axx * ayy - axy * axy)
    bxx, bxy, byy = ayy * rdet, -axy * rdet, axx * rdet
    qx, qy = px - mjx, py - mjy
    vx, vy = bxx * qx + bxy * qy, bxy * qx + byy * qy
    m = qx * vx + qy * vy
    s = d1 * np.exp(-half * d2 * m)
    jx, jy = t_y - py, px - t_x                          # K R mu
    zx, zy = two * (u * vy - sxy * vx), two * (u * vx + sxy * vy)      # Z_theta v
    rx, ry = jx - zx, jy - zy
    ct = (vx * jx + vy * jy) - half * (vx * zx + vy * zy)
    ux, uy = bxx * rx + bxy * ry, bxy * rx + byy * ry     # B r_theta
    hxx, hxy, hyy, hxt, hyt, htt = bxx, bxy, byy, ux, uy, rx * ux + ry * uy
    if prm.hessian_mode == O.HESSIAN_NEWTON:
        hxx = hxx - d2 * vx * vx
        hxy = hxy - d2 * vx * vy
        hyy = hyy - d2 * vy * vy
        hxt = hxt - d2 * vx * ct
        hyt = hyt - d2 * vy * ct
        # v' j_thth - 1/2 v' Z_thth v with j_thth = -R mu = (t - p'), Z_thth = -4 [[u, Sxy], [Sxy, -u]]
        htt = htt - d2 * ct * ct + (vx * (t_x - px) + vy * (t_y - py)) + two * (u * (vx * vx - vy * vy) + two * sxy * vx * vy)
    w = s * d2
    f64sum = lambda a: float(np.sum((w * a).astype(np.float64)))
    g = np.array([f64sum(vx), f64sum(vy), f64sum(ct)])
    h = [f64sum(a) for a in (hxx, hxy, hyy, hxt, hyt, htt)]
    Hm = np.array([[h[0], h[1], h[3]], [h[1], h[2], h[4]], [h[3], h[4], h[5]]])
    return Hm, g, float(np.sum(s.astype(np.float64))), int(hit.sum())


def score(tgt, comps, pose, prm) -> float:
    return evaluate(tgt, comps, pose, prm)[2]


def align(tgt: O.Grid2D, comps: Components, init_pose, prm: O.NdtParams, mirror32: bool = False, trace: list | None = None):
    """The loop of oracle.ndt2d.align over the map-to-map terms; the result's H, g, score, n_hit are the last evaluation's."""
    pose = tuple(float(v) for v in init_pose)
    it = 0
    if comps.n < 1 or tgt.n_valid < 1:
        return {"pose": pose, "H": np.zeros((3, 3)), "g": np.zeros(3), "score": 0.0, "n_hit": 0, "iterations": 0,
                "status": O.NDT_TOO_FEW_CELLS}
    ls = {} if prm.line_search > 0 else None
    while True:
        H, g, sc, n_hit = evaluate(tgt, comps, pose, prm, mirror32)
        if trace is not None:
            trace.append({"pose": pose, "H": H.copy(), "g": g.copy(), "score": sc, "n_hit": n_hit})
        pose, it, status, done = O.gn_update(pose, H, g, n_hit, it, prm, sc, ls)
        if done:
            return {"pose": pose, "H": H, "g": g, "score": sc, "n_hit": n_hit, "iterations": it, "status": status}


# ---- how two evaluations are compared (the normalisation tests/test_gpu_ndt2d.py uses for points) -------------
def eval_diffs(a, b):
    """(H, g, score) differences of evaluation a against the reference b, each relative to its natural scale:
    H to its largest entry, g to sqrt(H_ii * score) (its entries cancel), the score to itself."""
    Ha, ga, sa, _ = a
    Hb, gb, sb, _ = b
    hs = np.abs(Hb).max()
    gs = np.sqrt(np.abs(np.diag(Hb)) * max(sb, 1.0)) + 1e-30
    return float(np.abs(Ha - Hb).max() / hs), float(np.max(np.abs(ga - gb) / gs)), abs(sa - sb) / sb


EVAL_FLOOR = 2e-5       # the project's bound on H / g against the mirror oracle


def eval_bounds(cases, prm_of):
    """The GPU tests' bound on (H, g, score), measured from this restatement alone: 4 x the largest
    float32-vs-float64 difference over `cases` = [(tgt, comps, pose, name)], floored at EVAL_FLOOR.
    Returns (bounds [3], measured [3])."""
    worst = np.zeros(3)
    for tgt, comps, pose, name in cases:
        prm = prm_of(name)
        d = eval_diffs(evaluate(tgt, comps, pose, prm, mirror32=True), evaluate(tgt, comps, pose, prm))
        worst = np.maximum(worst, d)
    return np.maximum(4.0 * worst, EVAL_FLOOR), worst
