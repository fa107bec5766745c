"""Scenes and shared checks of the submap-coarsening GPU tests (test_gpu_coarsen_map.py, test_gpu_coarsen_map3d.py)."""
import numpy as np

import map_coarsen_ref as R


def lattice_cloud(seed, k0, ext, c, n, hole=None, bits=11):
    """n points with coordinates that are odd multiples of 2^-bits (every float32 step of the binning is exact, no point
    on a cell boundary), spread over the interior of the fine lattice with origin cell k0[a] and ext[a] cells per axis
    so that ndt*_set_target derives exactly that lattice: points sit in the first and the last interior cell of every
    axis (the interior cells next to the ring on all sides).  hole = (lo, hi): no point with all coordinates inside."""
    rng = np.random.default_rng(seed)
    dim = len(k0)
    lo = np.array([(k0[a] + 1) * c for a in range(dim)])
    hi = np.array([(k0[a] + ext[a] - 1) * c for a in range(dim)])
    u = rng.uniform(0.0, 1.0, size=(n, dim))
    side = max(dim * 8, n // 10)                       # points pressed against each face
    for j in range(side):
        a = j % dim
        u[j, a] = (0.3 * c / (hi[a] - lo[a])) * rng.uniform(0.1, 1.0) if (j // dim) % 2 == 0 else 1.0 - (0.3 * c / (hi[a] - lo[a])) * rng.uniform(0.1, 1.0)
    p = lo + u * (hi - lo)
    m = np.floor(p * 2.0 ** (bits - 1)).astype(np.int64)
    pts = ((2 * m + 1) * 2.0 ** -bits).astype(np.float32)
    if hole is not None:
        inside = np.all((pts >= np.array(hole[0])) & (pts < np.array(hole[1])), axis=1)
        pts = pts[~inside]
    origin, got = R.grid_geometry(pts, c)
    assert got == list(ext) and [int(np.rint(float(o) / c)) for o in origin] == list(k0), (got, origin)
    return pts


def assert_lattice_is_awkward(k0, ext, f):
    """What the issue asks of the fine extents: origin cell negative and no multiple of f, interior extent no multiple."""
    for a in range(len(k0)):
        assert k0[a] < 0 and k0[a] % f != 0 and (ext[a] - 2) % f != 0, (a, k0[a], ext[a])


def bins_alike(pts, c, f):
    """True when the float32 binning puts every point's coarse cell where the lattice puts its fine cell's parent, and
    the coarse lattice is the one ndt*_set_target derives at f c (asserted by the tests before they compare with it)."""
    of, ef = R.grid_geometry(pts, c)
    oc, ec = R.grid_geometry(pts, f * c)
    _, idf, _ = R.blob_from_points(pts, c)
    _, idc, _ = R.blob_from_points(pts, f * c)
    ok = True
    for a in range(pts.shape[1]):
        _, K0, off, extent = R.coarsen_axis(of[a], c, ef[a], f)
        ok = ok and extent == ec[a] and np.float32(K0 * c) == oc[a] and np.array_equal((off + idf[:, a]) // f, idc[:, a])
    return bool(ok)


def same_grid(a, b):
    for x, y in zip(a.grid(), b.grid()):
        assert np.array_equal(x, y)
    ia, ib = a.grid_info(), b.grid_info()
    for fld, _ in ia._fields_:
        assert getattr(ia, fld) == getattr(ib, fld), fld


def same_result(a, b):
    assert (tuple(a.pose) == tuple(b.pose) and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g) and a.score == b.score and
            a.iterations == b.iterations and a.n_hit == b.n_hit and a.status == b.status), (a, b)


def clamp_was_needed(fine_blob, f):
    """Does the coarsening of this blob raise some diagonal second sum (the degenerate-cell clamp)?"""
    return not np.array_equal(R.map_coarsen_ref(fine_blob, f), R.map_coarsen_ref(fine_blob, f, clamp=False))
