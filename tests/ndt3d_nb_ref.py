"""Float64 restatement of the 3D point-to-map terms over a neighbourhood of voxels (docs/ALGORITHM.md 2.25):
neighbourhood 1 is oracle.ndt3d.evaluate3, neighbourhood 7 adds the six face neighbours of the point's own voxel.

The formulas are evaluate3's, summed over the candidate list; the grid is oracle.ndt3d's (build_grid3), untouched.
With mirror32 the image p' = R p + t and the own-voxel index follow the device's float32 chain (image_row3 and
voxel_of3 of csrc/ndt3d_kernels.hpp): every fmaf is one float64 multiply-add rounded to float32, innermost first, as
tests/score_poses_ref.py does for 2D; (p' - o) * inv_c is two float32 operations.  Terms and sums are float64.
"""
import numpy as np

from oracle import ndt3d as o

# own, -x, +x, -y, +y, -z, +z: the order of the contract (and of a device thread's additions)
CANDIDATES = ((0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
BORDER_ULPS = 4.0


def _r32(a):
    """rounded to float32, held as float64"""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _fmaf(a, b, c):
    return _r32(a * b + c)


def own_voxels3(grid, sx, sy, sz, pose, mirror32: bool):
    """(P64 [n,3], Pw [n,3], idx [n,3] int64, inside [n] bool, n_border): the points as float64, their images, the
    integer indices of their own voxels (0 where outside) and the inside test.  n_border counts the points whose
    f = (p' - o) * inv_c lies within BORDER_ULPS float32 ulps of an integer on some axis: those whose own voxel the
    float32 rounding of the image may flip."""
    P = np.stack([np.asarray(sx), np.asarray(sy), np.asarray(sz)], axis=1)
    R = o.rot_and_derivs(*pose[3:])[0]
    t = np.array(pose[:3], dtype=np.float64)
    dims = np.array(grid.dims)
    with np.errstate(invalid="ignore"):
        if mirror32:
            P64 = _r32(P)
            R32, t32 = _r32(R), _r32(t)
            x, y, z = P64[:, 0], P64[:, 1], P64[:, 2]
            Pw = np.stack([_fmaf(R32[r, 0], x, _fmaf(R32[r, 1], y, _fmaf(R32[r, 2], z, t32[r]))) for r in range(3)], axis=1)
            f = ((Pw.astype(np.float32) - grid.o.astype(np.float32)) * np.float32(grid.inv_c)).astype(np.float64)
        else:
            P64 = P.astype(np.float64)
            Pw = P64 @ R.T + t
            f = (Pw - grid.o.astype(np.float64)) * float(grid.inv_c)
        inside = np.all((f >= 0.0) & (f < dims), axis=1)               # false for a NaN image
        idx = np.where(inside[:, None], np.floor(np.where(inside[:, None], f, 0.0)), 0.0).astype(np.int64)
        ulp = np.spacing(np.abs(f).astype(np.float32)).astype(np.float64)
        near = np.abs(f - np.rint(f)) <= BORDER_ULPS * ulp
        n_border = int(np.any(near & np.isfinite(f), axis=1).sum())
    return P64, Pw, idx, inside, n_border


def evaluate3_nb(grid, sx, sy, sz, pose, prm, neighbourhood: int = 7, mirror32: bool = False):
    """(H [6,6], g [6], score, n_hit, n_border) of the scan at `pose`: evaluate3's terms, one per (point, candidate voxel
    with a valid record).  n_hit counts point-voxel hits.  A point whose image is outside the grid or not finite has
    no candidates at all; a candidate whose index leaves the grid is skipped."""
    assert neighbourhood in (1, 7)
    P64, Pw, idx, inside, n_border = own_voxels3(grid, sx, sy, sz, pose, mirror32)
    _, Ra, Rb, Rg = o.rot_and_derivs(*pose[3:])
    if mirror32:
        mean, icov = (r.astype(np.float64) for r in grid.records32())
        Ra, Rb, Rg = (_r32(M) for M in (Ra, Rb, Rg))
    else:
        mean, icov = grid.mean, grid.icov
    W, Hh, D = grid.dims
    dims = np.array(grid.dims)
    pts, keys = [], []
    for d in CANDIDATES[:neighbourhood]:
        j = idx + np.array(d)
        ok = inside & np.all((j >= 0) & (j < dims), axis=1)            # by index, never by key arithmetic
        key = np.where(ok, (j[:, 2] * Hh + j[:, 1]) * W + j[:, 0], 0)
        hit = ok & grid.valid[key]
        pts.append(np.nonzero(hit)[0])
        keys.append(key[hit])
    i, k = np.concatenate(pts), np.concatenate(keys)
    q = Pw[i] - mean[k]
    ic = icov[k]
    C = np.empty((k.size, 3, 3))
    C[:, 0, 0], C[:, 0, 1], C[:, 0, 2] = ic[:, 0], ic[:, 1], ic[:, 2]
    C[:, 1, 0], C[:, 1, 1], C[:, 1, 2] = ic[:, 1], ic[:, 3], ic[:, 4]
    C[:, 2, 0], C[:, 2, 1], C[:, 2, 2] = ic[:, 2], ic[:, 4], ic[:, 5]
    v = np.einsum("nij,nj->ni", C, q)
    m = np.einsum("ni,ni->n", q, v)
    s = prm.d1 * np.exp(-0.5 * prm.d2 * m)
    w = s * prm.d2
    p = P64[i]
    J = np.zeros((k.size, 3, 6))
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1.0
    J[:, :, 3] = p @ Ra.T
    J[:, :, 4] = p @ Rb.T
    J[:, :, 5] = p @ Rg.T
    g = np.einsum("n,nik,ni->k", w, J, v)
    H = np.einsum("n,nik,nil->kl", w, J, np.einsum("nij,njl->nil", C, J))
    if prm.hessian_mode == 1:
        Jv = np.einsum("nik,ni->nk", J, v)
        H = H - prm.d2 * np.einsum("n,nk,nl->kl", w, Jv, Jv)
        M = np.einsum("n,na,nb->ab", w, v, p)
        for (a, b), Rab in o.rot_second_derivs(*pose[3:]).items():
            t2 = float(np.sum(Rab * M))
            H[3 + a, 3 + b] += t2
            if a != b:
                H[3 + b, 3 + a] += t2
    return H, g, float(s.sum()), int(k.size), n_border


def align3_nb(grid, sx, sy, sz, init_pose, prm, neighbourhood: int = 7, mirror32: bool = False, trace=None):
    """oracle.ndt3d.align3's loop (gn_update3) around evaluate3_nb."""
    pose = tuple(float(v) for v in init_pose)
    it = 0
    if grid.n_valid < 1:
        return {"pose": pose, "H": np.zeros((6, 6)), "g": np.zeros(6), "score": 0.0, "n_hit": 0,
                "iterations": 0, "status": o.NDT_TOO_FEW_CELLS}
    ls = {} if prm.line_search > 0 else None
    while True:
        H, g, score, n_hit, _ = evaluate3_nb(grid, sx, sy, sz, pose, prm, neighbourhood, mirror32)
        if trace is not None:
            trace.append({"pose": pose, "H": H.copy(), "g": g.copy(), "score": score, "n_hit": n_hit})
        pose, it, status, done = o.gn_update3(pose, H, g, n_hit, it, prm, score, ls)
        if done:
            return {"pose": pose, "H": H, "g": g, "score": score, "n_hit": n_hit, "iterations": it,
                    "status": status}
