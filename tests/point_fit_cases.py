"""Scenes for the per-point fit tests: the committed fixtures (tests/golden/ndt2d_config1.npz, ndt3d_small.npz), their
scans tiled with small offsets to the size a test needs, and the injected points the contract names: NaN and +-inf
coordinates, points far outside the grid, points on the ring, points displaced off their cell's Gaussian."""
import os

import numpy as np

import point_fit_ref as F

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_M = {2: 5.99, 3: 7.81}          # chi-square 95 % for 2 and 3 degrees of freedom (see point_fit_ref: no hit within tolerance of either)
# a rotation-free pose with float32 translations, and the rotated ones: the fixture's final pose, one beyond |theta| = 2
# and, in 3D, steep_scene's
EXACT_POSE = {2: (0.09375, -0.078125, 0.0), 3: (0.015625, -0.203125, 0.046875, 0.0, 0.0, 0.0)}


def fixture(dim):
    g = np.load(os.path.join(HERE, "golden", "ndt2d_config1.npz" if dim == 2 else "ndt3d_small.npz"))
    ax = "xyz"[:dim]
    return dict(target=tuple(g["t" + a] for a in ax), source=tuple(g["s" + a] for a in ax),
                final_pose=tuple(float(v) for v in g["final_pose"]))


def far_pose(dim, final_pose):
    """A pose with |theta| > 2 (3D: the yaw): the final pose with 2.5 rad added to the angle.  The scan turns about the
    map's origin, and enough of it still lands on mapped cells for a mixed scene."""
    p = list(final_pose)
    p[-1] += 2.5
    return tuple(p)


STEEP = (0.7, -0.5, 2.1)            # tilted_cases.ATTITUDES["steep"]: roll and pitch where the sin roll sin pitch entries of R count


def steep_scene(fx):
    """The 3D fixture seen from a steeply tilted sensor frame -> (source, pose): the scan re-expressed, s' = Q' s with
    Q = R(final)' R(STEEP) in float64 and rounded to float32, and the pose (final translation, STEEP) that puts it where
    the final pose puts the original - the same images to float32 rounding, so the same mix of fits, misfits and misses,
    through a rotation matrix none of whose entries is near 0 or 1."""
    from oracle import ndt3d as o3
    final = fx["final_pose"]
    Q = o3.rot_and_derivs(*final[3:])[0].T @ o3.rot_and_derivs(*STEEP)[0]
    P = np.stack(fx["source"], axis=1).astype(np.float64) @ Q
    return tuple(np.ascontiguousarray(P[:, a].astype(np.float32)) for a in range(3)), tuple(final[:3]) + STEEP


def tiled(coords, n, step=0.004):
    """The scan extended to n points: copy j is the scan moved by (j step, -j step / 2[, j step / 4])."""
    base = len(coords[0])
    reps = -(-n // base)
    off = (step, -0.5 * step, 0.25 * step)
    out = []
    for a, c in enumerate(coords):
        c = np.asarray(c, dtype=np.float32)
        out.append(np.concatenate([c + np.float32(j * off[a]) for j in range(reps)])[:n].astype(np.float32))
    return tuple(out)


def to_source(world, pose, dim):
    """World points [k, dim] -> source-frame float32 coordinates under `pose` (the float64 inverse)."""
    R, t = F.rotation32(pose, dim)
    return ((np.asarray(world, dtype=np.float64) - t[None, :]) @ R).astype(np.float32)


def ring_points(rec, pose, k):
    """k source points whose images are centres of cells on the grid's outermost ring (grid 0)."""
    ext = np.array(rec.ext)
    idx = np.zeros((k, rec.dim))
    for j in range(k):
        idx[j] = [(j * 3 + 1) % e for e in ext]
        idx[j, j % rec.dim] = 0 if (j // rec.dim) % 2 == 0 else ext[j % rec.dim] - 1
    world = rec.origin[0].astype(np.float64)[None, :] + (idx + 0.5) * rec.cell
    return to_source(world, pose, rec.dim)


def minor_axis(rec, q, key):
    """Unit vectors [k, dim] along the least-variance axis of cells `key` of grid q (largest eigenvalue of Sigma^-1)."""
    dim = rec.dim
    C = np.zeros((len(key), dim, dim))
    for p, (a, b) in enumerate(F.PAIRS[dim]):
        C[:, a, b] = C[:, b, a] = rec.icov[q][key, p]
    w, v = np.linalg.eigh(C)
    return v[:, :, -1]


def displaced(rec, coords, pose, idx, dist=0.25):
    """The points idx of the scan - hits - moved `dist` along the minor axis of the cell they hit (with four grids: of
    the first grid whose cell is valid), as source points [len(idx), dim] float32."""
    from oracle import ndt2d as o2, ndt3d as o3
    dim = rec.dim
    X = np.stack([np.asarray(c, dtype=np.float32)[idx] for c in coords], axis=1).astype(np.float64)
    R, t = F.rotation32(pose, dim)
    img = X @ R.T + t[None, :]
    img32 = img.astype(np.float32)
    axis = np.zeros_like(img)
    done = np.zeros(len(idx), bool)
    for q in range(rec.ngrid):
        o = rec.origin[q]
        if dim == 2:
            key, inside = o2.cell_keys32(img32[:, 0], img32[:, 1], o[0], o[1], rec.inv_c, rec.ext[0], rec.ext[1])
        else:
            key, inside = o3.cell_keys3(img32, o, rec.inv_c, rec.ext)
        take = inside & rec.valid[q][key] & ~done
        axis[take] = minor_axis(rec, q, key[take])
        done |= take
    assert done.all(), "displaced(): the chosen points must hit a valid cell"
    return to_source(img + dist * axis, pose, dim)


def displaced_outliers(rec, coords, pose, k, dist=0.25, misfit_only=False):
    """k points of the scan that hit the map, moved `dist` along the minor axis of their cell, chosen so that the
    REFERENCE classes every moved point MISS or MISFIT with its tolerance to spare (a cell whose thin axis is wider than
    dist / sqrt(max_m), or a neighbour cell that takes the moved point in, lets it fit: those are passed over).  Evenly
    spread over the scan.  misfit_only: only points whose moved image still lies in a valid cell - a moved point that
    leaves the mapped cells is a MISS, which a selection of fit | miss keeps by design.
    -> (their indices in the scan, the moved points [k, dim] float32)."""
    dim = rec.dim
    r = F.fit_ref(rec, coords, pose, MAX_M[dim])
    hits = np.flatnonzero(r["hit"])
    moved = displaced(rec, coords, pose, hits, dist)
    rm = F.fit_ref(rec, tuple(moved[:, a] for a in range(dim)), pose, MAX_M[dim])
    firm = ~rm["near"] & (((rm["cls"] == F.MISS) & (not misfit_only)) | ((rm["cls"] == F.MISFIT) & (rm["m"] - MAX_M[dim] > rm["tol"])))
    ok = np.flatnonzero(firm)
    assert len(ok) >= k, f"only {len(ok)} of {len(hits)} moved hits are firmly outside the fit"
    take = ok[np.linspace(0, len(ok) - 1, k).astype(np.int64)]
    return hits[take], moved[take]


def mixed_scan(rec, source, pose, n, n_displaced=40):
    """A scan of n points for the fit tests: the source tiled to n, with - at fixed places spread over all tiles -
    NaN / +inf / -inf coordinates, far points, ring points and displaced hits written over it.
    -> (coords, dict of the index arrays of what was injected)."""
    dim = rec.dim
    coords = [c.copy() for c in tiled(source, n)]
    ref = F.fit_ref(rec, coords, pose, MAX_M[dim])
    hits = np.flatnonzero(ref["hit"])
    slots = np.linspace(0, n - 1, 64 + n_displaced).astype(np.int64)
    slots = np.unique(slots)
    bad, far, ring, disp = slots[0:64:4], slots[1:64:4], slots[2:64:4], slots[64:]
    vals = (np.nan, np.inf, -np.inf)
    for j, i in enumerate(bad):
        coords[j % dim][i] = vals[j % 3]
    for j, i in enumerate(far):
        for a in range(dim):
            coords[a][i] = np.float32((-1.0) ** (j + a) * (1.0e4 + 977.0 * j))
    rp = ring_points(rec, pose, len(ring))
    for a in range(dim):
        coords[a][ring] = rp[:, a]
    if len(hits) and len(disp):
        _, dpnt = displaced_outliers(rec, tiled(source, n), pose, len(disp))
        for a in range(dim):
            coords[a][disp] = dpnt[:, a]
    return tuple(coords), dict(bad=bad, far=far, ring=ring, displaced=disp)


# ---------------------------------------------------------------------------------------------- device-side helpers
def matcher(dim, ngrid=1, **kw):
    """A matcher of the fixture's target (default parameters; ngrid 4: overlapping grids)."""
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D
    m = NdtMatcher2D(overlap_grids=ngrid, **kw) if dim == 2 else NdtMatcher3D(**kw)
    m.set_target(*fixture(dim)["target"])
    return m


def dev(coords):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in coords)


def raw_fit(m, dcoords, pose, max_m, d_m=None, d_cls=None, n=None):
    """ndt*_fit_points_dev as the C ABI has it (null arrays allowed) -> (status, L.PointFit)."""
    import ctypes as C
    from gtsam_ndt_amd import _lib as L
    fit = L.PointFit()
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    m.wait_stream()
    st = m._c.fit_points_dev(m._h, *[ptr(c) for c in dcoords], dcoords[0].numel() if n is None else n,
                             None if pose is None else m._dim.pose(pose), float(max_m), ptr(d_m), ptr(d_cls), C.byref(fit))
    return st, fit


def raw_select(m, dcoords, pose, max_m, keep, out, index=None, n=None, fit=True):
    """ndt*_select_points_dev as the C ABI has it, into the caller's output tensors -> (status, L.PointFit)."""
    import ctypes as C
    from gtsam_ndt_amd import _lib as L
    f = L.PointFit()
    ptr = lambda t: None if t is None else t.data_ptr()
    m.wait_stream()
    st = m._c.select_points_dev(m._h, *[ptr(c) for c in dcoords], dcoords[0].numel() if n is None else n,
                                None if pose is None else m._dim.pose(pose), float(max_m), int(keep), *[ptr(o) for o in out],
                                ptr(index), C.byref(f) if fit else None)
    return st, f


def fit_tuple(f):
    return (int(f.n_invalid), int(f.n_miss), int(f.n_misfit), int(f.n_fit), int(f.n_selected))
