"""Reference for ndt2d/ndt3d_fit_points* and _select_points_dev (docs/ALGORITHM.md section 2.19) in float64 numpy.

Inputs: cell records as float32 values (the device's own, records_of(matcher); or an oracle grid's, for the CPU test of
this file), the grid geometry, a scan, a pose, max_m.  Output: per point the class, m = q' Sigma^-1 q (the least over the
grids whose cell is valid), and what the tolerance of a comparison with the device needs.

Image points.  The rotation is the one the kernels use - cos / sin (3D: the nine products of R = Rz Ry Rx, in the
kernels' order) formed in float64 and rounded to float32 - applied in float64.  exact=True is for poses without rotation
whose translation holds float32 values: R p + t is then ONE float32 addition per axis on the device, and numpy float32
reproduces the image point, hence the cell key, exactly.

Keys.  2D through oracle.ndt2d.cell_keys32 per grid (the device clamps onto the ring instead of testing; the ring holds
no valid cell, so the hits are the same), 3D through oracle.ndt3d.cell_keys3 (0 <= f < extent).

THE TOLERANCE of a device m against this m, per hit (K = 8 in 2D, 10 in 3D):

    |m_dev - m_ref| <= K 2^-24 M_abs,   M_abs = sum_ab |c_ab| |q_a| |q_b|

The float32 sequence has 6 (2D: two subtractions, three fmas, two multiplies, of which q's two roundings enter twice)
resp. 8 first-order roundings, each at most 2^-24 of a partial sum bounded by M_abs; the rest is headroom for second-order
terms.  With four grids both sides take a minimum over the same grids, and |min a - min b| <= max |a_q - b_q|: the
tolerance is the largest of the valid grids'.

At a rotated pose the device's image point differs from this one by at most dp = 2^-23 (sum |coord| + max |t|) per axis
(the roundings of the nested fmas), and m(q + d) - m(q) = 2 v'd + d'Cd with v = Cq adds

    2 |v|_1 dp + |C|_1 dp^2          (|C|_1: the sum of |c_ab| over the full matrix)

The cell itself is exact at a rotated pose as well: the key is taken from the device's own float32 image, the fmaf chain
with a correctly rounded fma (tests/seam_ref.py image2d / image3d).  `near` is therefore empty at every pose; it stays in
the result for the comparisons that read it.
"""
import math
from dataclasses import dataclass

import numpy as np

from oracle import ndt2d as o2
from oracle import ndt3d as o3

import seam_ref as S

INVALID, MISS, MISFIT, FIT = 0, 1, 2, 3
K_ROUND = {2: 8.0, 3: 10.0}
PAIRS = {2: ((0, 0), (0, 1), (1, 1)), 3: ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))}
EPS24, EPS23, EPS22 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22


@dataclass
class Records:
    """The grids of one handle: float32 values throughout (kept as float64 where arithmetic follows)."""
    dim: int
    ext: tuple                # (W, H) | (W, H, D)
    origin: np.ndarray        # float32 [ngrid, dim]
    inv_c: np.float32
    valid: np.ndarray         # bool [ngrid, cells]
    mean: np.ndarray          # float64 [ngrid, cells, dim]
    icov: np.ndarray          # float64 [ngrid, cells, nsym]

    @property
    def ngrid(self):
        return self.origin.shape[0]

    @property
    def cell(self):
        return 1.0 / float(self.inv_c)


def records_of(m):
    """The device's own records of a matcher: geometry from grid_info() and the save_map header (the origins of all
    grids), grid 0 from m.grid().  ndt2d_get_grid hands out grid 0 only; with overlap_grids = 4 the records of grids 1 - 3
    are the documented device formula on the blob's exact sums in float64 (cell_record_ref.records_float64), rounded to
    float32 - the values the device stores, up to a float64 rounding in front of the float32 one."""
    import cell_record_ref as C
    import map_coarsen_ref as R
    info = m.grid_info()
    blob = m.save_map()
    h, _ = R.parse(blob)
    dim = h["dims"]
    ext = (h["width"], h["height"], h["depth"])[:dim]
    ng = h["ngrid"]
    ncell = int(np.prod(ext))
    origin = np.asarray(h["origin"], dtype=np.float32)[:ng, :dim]
    nsym = len(PAIRS[dim])
    mean = np.zeros((ng, ncell, dim))
    icov = np.zeros((ng, ncell, nsym))
    _, mean0, icov0 = m.grid()
    if ng > 1:
        r = C.records_float64(blob, int(m.params.min_points), float(m.params.eig_ratio))
        mean[:] = r["mean"].astype(np.float32).reshape(ng, ncell, dim)
        icov[:] = r["icov"].astype(np.float32).reshape(ng, ncell, nsym)
    mean[0], icov[0] = mean0, icov0
    valid = icov[:, :, 0] > 0.0                         # an invalid cell's record is zero; Sigma^-1 is positive definite
    mean[~valid] = 0.0
    return Records(dim, ext, origin, np.float32(info.inv_cell), valid, mean, icov)


def records_of_oracle(grids):
    """The same from oracle grids (a list of oracle.ndt2d.Grid2D, or one oracle.ndt3d.Grid3D): float32 records."""
    if isinstance(grids, o3.Grid3D):
        g = grids
        mean, icov = g.records32()
        return Records(3, tuple(g.dims), np.asarray(g.o, np.float32)[None], np.float32(g.inv_c), g.valid[None].copy(),
                       mean.astype(np.float64)[None], icov.astype(np.float64)[None])
    rec = [g.records32() for g in grids]
    g0 = grids[0]
    return Records(2, (g0.W, g0.H), np.array([[g.ox, g.oy] for g in grids], np.float32), np.float32(g0.inv_c),
                   np.stack([g.valid for g in grids]), np.stack([r[0].astype(np.float64) for r in rec]),
                   np.stack([r[1].astype(np.float64) for r in rec]))


def _wrap(t):
    return o2.wrap_angle(float(t))


def rotation32(pose, dim):
    """(R [dim, dim], t [dim]) as the kernels hold them: float32 values, here in float64."""
    f32 = lambda v: float(np.float32(v))
    if dim == 2:
        th = _wrap(pose[2])
        c, s = f32(math.cos(th)), f32(math.sin(th))
        return np.array([[c, -s], [s, c]]), np.array([f32(pose[0]), f32(pose[1])])
    R = np.array(S.rot3d_entries(*pose[3:6])).reshape(3, 3)          # wrapped angles, the nine products of csrc/ndt_pose.hpp
    return R.astype(np.float32).astype(np.float64), np.array([f32(v) for v in pose[:3]])


def is_exact_pose(pose, dim):
    ang = pose[2:3] if dim == 2 else pose[3:6]
    return all(float(v) == 0.0 for v in ang) and all(float(np.float32(v)) == float(v) for v in pose[:dim])


def fit_ref(rec: Records, coords, pose, max_m, exact=False):
    """-> dict over the scan's points: cls uint8, m float64 (+inf: miss, NaN: invalid), hit bool, tol float64 (the m
    tolerance above, rotated terms included unless exact), near bool (always False: the key is exact
    at every pose), m_abs."""
    dim = rec.dim
    P = np.stack([np.asarray(c, dtype=np.float32) for c in coords[:dim]], axis=1)
    n = P.shape[0]
    finite = np.isfinite(P).all(axis=1)
    X = np.where(finite[:, None], P, np.float32(0)).astype(np.float32)
    R, t = rotation32(pose, dim)
    if exact:
        assert is_exact_pose(pose, dim), "exact=True needs a pose without rotation and a float32 translation"
        img = (X + t.astype(np.float32)[None, :]).astype(np.float32).astype(np.float64)      # one float32 add per axis
        dp = np.zeros(n)
    else:
        img = X.astype(np.float64) @ R.T + t[None, :]
        dp = EPS23 * (np.abs(X.astype(np.float64)).sum(axis=1) + np.abs(t).max())
    if exact:
        img32 = img.astype(np.float32)
    else:
        # the key comes from the device's own image: the fmaf chain of ALGORITHM 2.4 / 2.6 with a correctly rounded fma
        # (tests/seam_ref.py), so the cell is exact at a rotated pose too; img (float64) and dp remain for the m tolerance
        chain = S.image2d(X[:, 0], X[:, 1], pose) if dim == 2 else S.image3d(X[:, 0], X[:, 1], X[:, 2], pose)
        img32 = np.stack(chain, axis=1)
    ng = rec.ngrid
    m_q = np.full((ng, n), np.inf)
    tol_q = np.zeros((ng, n))
    mabs_q = np.zeros((ng, n))
    near = np.zeros(n, bool)
    for q in range(ng):
        o = rec.origin[q]
        if dim == 2:
            key, inside = o2.cell_keys32(img32[:, 0], img32[:, 1], o[0], o[1], rec.inv_c, rec.ext[0], rec.ext[1])
        else:
            key, inside = o3.cell_keys3(img32, o, rec.inv_c, rec.ext)
        hit = inside & rec.valid[q][key] & finite
        k = key[hit]
        qv = img[hit] - rec.mean[q][k]
        C = np.zeros((k.size, dim, dim))
        for p, (a, b) in enumerate(PAIRS[dim]):
            C[:, a, b] = C[:, b, a] = rec.icov[q][k, p]
        v = np.einsum("kab,kb->ka", C, qv)
        m_q[q, hit] = np.einsum("ka,ka->k", qv, v)
        mabs = np.einsum("kab,ka,kb->k", np.abs(C), np.abs(qv), np.abs(qv))
        mabs_q[q, hit] = mabs
        d = dp[hit]
        tol_q[q, hit] = K_ROUND[dim] * EPS24 * mabs + 2.0 * np.abs(v).sum(axis=1) * d + np.abs(C).sum(axis=(1, 2)) * d * d
    m = m_q.min(axis=0)
    hit = np.isfinite(m)
    cls = np.full(n, MISS, np.uint8)
    cls[hit & (m.astype(np.float32) <= np.float32(max_m))] = FIT
    cls[hit & ~(m.astype(np.float32) <= np.float32(max_m))] = MISFIT
    cls[~finite] = INVALID
    m = np.where(finite, m, np.nan)
    return dict(cls=cls, m=m, hit=hit, tol=tol_q.max(axis=0), near=near & finite, m_abs=mabs_q.max(axis=0), finite=finite)


def keep_mask(cls, keep):
    """bool [n]: the points whose class is in `keep` (a mask of 1 << class)."""
    return ((int(keep) >> np.asarray(cls).astype(np.int64)) & 1).astype(bool)


def select_ref(coords, cls, keep):
    """Stable selection: (coords at the kept indices, the indices ascending)."""
    idx = np.flatnonzero(keep_mask(cls, keep))
    return tuple(np.asarray(c)[idx] for c in coords), idx


def counts(cls):
    c = np.bincount(np.asarray(cls, dtype=np.int64), minlength=4)
    return dict(n_invalid=int(c[0]), n_miss=int(c[1]), n_misfit=int(c[2]), n_fit=int(c[3]))


def compare(ref, m_dev, cls_dev, max_m, cap=0.01):
    """The comparison of tests 1 and 2, as a dict of figures and a list of failures (empty = pass).
    - invalid / miss / hit agree at every point that is not `near` (exact poses have no near points);
    - |m_dev - m_ref| <= tol at every hit that is not near;
    - fit / misfit agree wherever |m_ref - max_m| > tol;
    - the excused points (near, or within tol of the threshold) are at most `cap` of the hits."""
    m_dev = np.asarray(m_dev, dtype=np.float64)
    cls_dev = np.asarray(cls_dev)
    cls, m, hit, tol, near = ref["cls"], ref["m"], ref["hit"], ref["tol"], ref["near"]
    fails = []
    sure = ~near
    coarse = lambda c: np.minimum(c, 2)                                   # invalid, miss, hit
    bad = sure & (coarse(cls_dev) != coarse(cls))
    if bad.any():
        fails.append(f"{int(bad.sum())} points differ in invalid / miss / hit, first {int(np.flatnonzero(bad)[0])}")
    both = sure & hit & (cls_dev >= MISFIT)
    err = np.abs(m_dev[both] - m[both])
    worst = float((err / np.maximum(tol[both], 1e-300)).max()) if both.any() else 0.0
    if (err > tol[both]).any():
        fails.append(f"{int((err > tol[both]).sum())} hits beyond the m tolerance, worst {worst:.3f} of it")
    edge = hit & (np.abs(m - float(np.float32(max_m))) <= tol)
    firm = both & ~edge
    if (cls_dev[firm] != cls[firm]).any():
        fails.append(f"{int((cls_dev[firm] != cls[firm]).sum())} firm hits differ in fit / misfit")
    # stored m of the other classes
    miss = sure & (cls == MISS) & (cls_dev == MISS)
    if not np.all(np.isposinf(m_dev[miss])):
        fails.append("a miss does not store +inf")
    if not np.all(np.isnan(m_dev[cls_dev == INVALID])):
        fails.append("an invalid point does not store NaN")
    excused = int(((near & (hit | (cls_dev >= MISFIT))) | edge).sum())
    n_hit = int(hit.sum())
    if excused > cap * n_hit:
        fails.append(f"{excused} excused points of {n_hit} hits: above {cap:.0%}")
    return dict(n_hit=n_hit, excused=excused, worst_m=worst, n_near=int(near.sum()), n_edge=int(edge.sum())), fails
