"""The voxel-grid scan filter of docs/ALGORITHM.md section 2.24 restated in numpy: what ndt2d/ndt3d_voxel_filter compute on
the device, for a caller without one and for the tests.  The same float64 operations in the same order, integer sums per
voxel, one fused multiply-add and one rounding to float32 per output coordinate, so the device's output equals this one
bit for bit.

The lattice is absolute: voxel index i = floor(x / leaf) per axis, whatever the cloud's bounding box.  Per point and axis
  i = floor(x / leaf)                   one IEEE division
  centre = (i + 0.5) leaf               one rounded product
  U = rint((x - centre) (2^22 / leaf))  the submap's quantisation (section 2.2), here leaf 2^-22
per occupied voxel n and the sum of U per axis (int64), and the output mu = fma(sum U, leaf / (n 2^22), centre) as float32.
A point with a non-finite coordinate or an |i| >= 2^30 is skipped.  Output order: ascending (iz, iy, ix), ix fastest.
"""
from __future__ import annotations

import numpy as np

FIX = 4194304.0            # 2^22
INDEX_LIMIT = 1 << 30      # |i| below this


def _two_sum(a, b):
    """s = fl(a + b) and the exact error e: a + b = s + e."""
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _two_prod(a, b):
    """p = fl(a b) and the exact error e (Dekker's product on Veltkamp's split; no overflow for the sizes here)."""
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _add_round_to_odd(a, b):
    """a + b rounded to odd: the exact sum where it is a double, else its neighbour with an odd significand."""
    s, e = _two_sum(a, b)
    even = (s.view(np.int64) & 1) == 0
    toward = np.where(e > 0.0, np.inf, -np.inf)
    return np.where((e != 0.0) & even, np.nextafter(s, toward), s)


def fma(a, b, c):
    """a b + c with one rounding, elementwise on float64 arrays (numpy has none): the product and the first sum are
    kept exactly as pairs, the sum of the two small parts is rounded to odd, and the last addition then rounds to
    nearest as the exact sum would (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums", 2008).
    No overflow or underflow may occur on the way, which holds for the magnitudes of this module."""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    uh, ul = _two_prod(a, b)
    th, tl = _two_sum(c, uh)
    return th + _add_round_to_odd(tl, ul)


def lattice(coords, leaf: float):
    """Per point of coords [n, dim]: (valid [n] bool, i [n, dim] int64, centre [n, dim], U [n, dim] int64); the last three
    are zero where a point is not valid."""
    x = np.asarray(coords, dtype=np.float32).astype(np.float64)
    leaf = float(leaf)
    if not (np.isfinite(leaf) and leaf > 0.0):
        raise ValueError("leaf must be finite and positive")
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor(x / leaf)
        valid = (np.isfinite(x) & (np.abs(f) < float(INDEX_LIMIT))).all(axis=1)
    f = np.where(valid[:, None], f, 0.0)
    x = np.where(valid[:, None], x, 0.0)
    i = f.astype(np.int64)
    centre = (f + 0.5) * leaf
    U = np.rint((x - centre) * (FIX / leaf)).astype(np.int64)
    keep = valid[:, None]
    return valid, i, np.where(keep, centre, 0.0), np.where(keep, U, 0)


def voxel_sums(coords, leaf: float):
    """The occupied voxels in the contract's order: (index [m, dim] int64, n [m] int64, sum U [m, dim] int64, invalid
    points)."""
    coords = np.asarray(coords, dtype=np.float32)
    if coords.ndim != 2 or coords.shape[1] not in (2, 3):
        raise ValueError("coords must be [n, 2] or [n, 3]")
    valid, i, _, U = lattice(coords, leaf)
    i, U = i[valid], U[valid]
    dim = coords.shape[1]
    if i.shape[0] == 0:
        return np.zeros((0, dim), np.int64), np.zeros(0, np.int64), np.zeros((0, dim), np.int64), int((~valid).sum())
    index, inverse = np.unique(i[:, ::-1], axis=0, return_inverse=True)      # rows (iz, iy, ix), ascending
    inverse = np.asarray(inverse).reshape(-1)
    n = np.bincount(inverse, minlength=index.shape[0]).astype(np.int64)
    S = np.zeros((index.shape[0], dim), np.int64)
    np.add.at(S, inverse, U)
    return index[:, ::-1], n, S, int((~valid).sum())


def voxel_filter(coords, leaf: float, min_points: int = 1, with_info: bool = False):
    """coords [n, dim] (dim 2 or 3) -> (points [m, dim] float32, counts [m] uint32): the centroid and the point count of
    every voxel with at least min_points points, in ascending lattice order.  with_info: also a dict n_invalid / n_voxels /
    n_out as ndt_voxel_filter_info."""
    if int(min_points) < 1:
        raise ValueError("min_points must be at least 1")
    leaf = float(leaf)
    index, n, S, n_invalid = voxel_sums(coords, leaf)
    kept = n >= int(min_points)
    index, nk, S = index[kept], n[kept], S[kept]
    centre = (index.astype(np.float64) + 0.5) * leaf
    step = leaf / (nk.astype(np.float64) * FIX)
    mu = fma(S.astype(np.float64), step[:, None], centre)
    out = mu.astype(np.float32), nk.astype(np.uint32)
    if with_info:
        return out + (dict(n_invalid=n_invalid, n_voxels=int(n.size), n_out=int(nk.size)),)
    return out
