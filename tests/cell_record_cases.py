"""The catalogue of cells behind tests/test_cell_record_ref.py and tests/test_gpu_cell_records.py: where the step from
a cell's exact sums to its records (mean, clamped Sigma^-1, clamped Sigma) can go wrong.

LATTICE catalogues ('lattice2', 'lattice3').  A case is a small multiset of integer offsets U in [-2^21, 2^21)^dim (the
quantised cell-centred coordinates of docs/ALGORITHM.md 2.2).  One case is laid into each interior cell of a lattice with
c = 0.5, origin a multiple of c and every cell inside |x| < 2 m (8 x 8 interior cells in 2D, 6 x 6 x 6 inside
|x| < 1.5 m in 3D), so that centre + U 2^-23 is exactly a float32.  The catalogue therefore exists twice: as a float32
cloud for set_target, and as a blob forged from the U's alone for load_map (it passes cell_sums_plausible by
construction; test_cell_record_ref checks that, and that binning the cloud gives the same bytes).

FAR catalogues ('far2_0'.., 'far3_0'..): c = 0.3 (a scale S that is no power of two) around (+-700, +-700[, +-40]),
arbitrary float32 points - walls, duplicates, anisotropic blobs - one small cloud per sign combination; the U's follow
from map_coarsen_ref.blob_from_points.

PARAMS are the (min_points, eig_ratio) pairs every catalogue has a committed expectation for
(tests/golden/cell_records.npz, written by tests/golden/make_cell_records_golden.py)."""
import functools
import math
import os

import numpy as np

import map_coarsen_ref as R

PARAMS = ((2, 1e-3), (3, 1e-2), (6, 0.1), (2, 1e-6), (3, 1.0))
LIM = 1 << 21
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cell_records.npz")


# ---------------------------------------------------------------------------------------------- integer helpers
def _three_squares(m):
    b = math.isqrt(m)
    while b >= 0:
        r = m - b * b
        c = math.isqrt(r)
        while c >= 0 and 2 * c * c >= r:
            d = math.isqrt(r - c * c)
            if d * d == r - c * c:
                return [b, c, d]
            c -= 1
        b -= 1
    return None


def squares_summing_to(T, m, amax):
    """Positive integers <= amax whose squares sum to T exactly: m equal values, then at most four for the remainder."""
    b = min(amax, math.isqrt(T // m))
    out = [b] * m if b else []
    rem = T - m * b * b
    a = math.isqrt(rem)
    while True:
        rest = _three_squares(rem - a * a)
        if rest is not None:
            break
        a -= 1
    out += [v for v in [a] + rest if v]
    assert sum(v * v for v in out) == T and max(out, default=0) <= amax
    return out


FRAME2 = ((3, 4), (-4, 3))                                  # orthogonal integer frames of equal length (5 and 3)
FRAME3 = ((1, 2, 2), (2, 1, -2), (2, -2, 1))
AXES2 = ((1, 0), (0, 1))
AXES3 = ((1, 0, 0), (0, 1, 0), (0, 0, 1))


def cross(frame, amax, ratios, m=4):
    """+-a e_0 for the m values a = amax, amax - 1, .., and along every further axis k points +-b e_k whose squares sum
    to ratios[k - 1] times the first axis' (rounded to an integer): eigenvalues exactly in the ratio of the integer sums,
    eigenvectors the frame.  Returns (U, the exact eigenvalue ratios as (numerator, denominator))."""
    long = [amax - t for t in range(m)]
    A = sum(a * a for a in long)
    pts, exact = [], []
    e = np.array(frame, dtype=np.int64)
    for a in long:
        pts += [a * e[0], -a * e[0]]
    for k, ratio in enumerate(ratios, start=1):
        T = max(int(round(A * ratio)), 1)
        for b in squares_summing_to(T, m, amax):
            pts += [b * e[k], -b * e[k]]
        exact.append((T, A))
    return np.array(pts, dtype=np.int64), exact


def _rounded_rotation(U, angles):
    U = np.asarray(U, dtype=np.float64)
    dim = U.shape[1]
    if dim == 2:
        c, s = math.cos(angles[0]), math.sin(angles[0])
        Rm = np.array([[c, -s], [s, c]])
    else:
        Rm = np.eye(3)
        for ax, t in enumerate(angles):
            c, s = math.cos(t), math.sin(t)
            i, j = [(1, 2), (0, 2), (0, 1)][ax]
            G = np.eye(3)
            G[i, i] = G[j, j] = c
            G[i, j], G[j, i] = -s, s
            Rm = G @ Rm
    return np.rint(U @ Rm.T).astype(np.int64)


def _random_cloud(rng, n, dim):
    scale = np.array([3e5, 3e3, 40.0][:dim])
    U = rng.normal(size=(n, dim)) * scale
    U = _rounded_rotation(U, rng.uniform(0, math.pi, 3)) + rng.integers(-200000, 200000, dim)
    return np.clip(U, -LIM, LIM - 4)


def _big_cell(dim):
    """2^20 points: an oblique anisotropic integer lattice."""
    if dim == 2:
        i, j = np.meshgrid(np.arange(-512, 512), np.arange(-512, 512), indexing="ij")
        i, j = i.ravel(), j.ravel()
        return np.stack([2000 * i - 300 * j, 1000 * i + 700 * j], axis=1).astype(np.int64)
    i, j, k = np.meshgrid(np.arange(-64, 64), np.arange(-64, 64), np.arange(-32, 32), indexing="ij")
    i, j, k = i.ravel(), j.ravel(), k.ravel()
    return np.stack([9000 * i - 2000 * j + 700 * k, 4000 * i + 6000 * j - 500 * k, -1000 * i + 800 * j + 3000 * k],
                    axis=1).astype(np.int64)


def lattice_cases(dim):
    """[(name, U int64 [n, dim])]."""
    rng = np.random.default_rng(20261019 + dim)
    Z = lambda *rows: np.array(rows, dtype=np.int64).reshape(-1, dim)
    frame, axes = (FRAME2, AXES2) if dim == 2 else (FRAME3, AXES3)
    e = np.array(frame, dtype=np.int64)
    pad = (0,) * (dim - 2)
    cases = []
    add = lambda name, U: cases.append((name, np.asarray(U, dtype=np.int64).reshape(-1, dim)))
    # counts around every min_points in use (2, 3, 6): n = 1, 2, 3, 5, 6
    generic = rng.integers(-900000, 900000, size=(6, dim))
    for n in (1, 2, 3, 5, 6):
        add(f"n{n}", generic[:n])
    add("coincident2", Z(*[(777, -12345) + (99,) * (dim - 2)] * 2))                        # trace 0: invalid
    add("coincident7", Z(*[(-LIM, LIM - 4) + (5,) * (dim - 2)] * 7))
    ks = np.arange(-7, 8)
    for a in range(dim):                                                                   # axis-aligned lines: rank 1
        add(f"line_axis{a}", ks[:, None] * 100000 * np.array(axes[a]))
    add("rect_wide", Z(*[(sx * 900000, sy * 1000) + pad for sx in (-1, 1) for sy in (-1, 1)]
                       + ([(0, 0, 30), (0, 0, -30)] if dim == 3 else [])))                 # vxy == 0, half_df > 0
    add("rect_tall", Z(*[(sx * 1000, sy * 900000) + pad for sx in (-1, 1) for sy in (-1, 1)]
                       + ([(0, 0, 30), (0, 0, -30)] if dim == 3 else [])))                 # vxy == 0, half_df < 0
    add("diag45", ks[:, None] * 100000 * np.array((1, 1) + pad))                           # half_df == 0, vxy > 0
    add("diag135", ks[:, None] * 100000 * np.array((1, -1) + pad))                         # half_df == 0, vxy < 0
    add("slope_2^-17", np.stack([ks * (1 << 17), ks] + [0 * ks] * (dim - 2), axis=1))
    add("line_oblique", ks[:, None] * 40000 * e[0])
    if dim == 3:
        g = np.array([(i, j) for i in range(-3, 4) for j in range(-3, 4)])
        add("plane_xy", np.stack([g[:, 0] * 200000, g[:, 1] * 150000, 0 * g[:, 0] + 4321], axis=1))
        add("plane_xz", np.stack([g[:, 0] * 200000, 0 * g[:, 0] - 77, g[:, 1] * 150000], axis=1))
        add("plane_oblique", g[:, :1] * 60000 * e[0] + g[:, 1:] * 45000 * e[1])
        add("diag111", ks[:, None] * 100000 * np.array((1, 1, 1)))
    corners = np.array(np.meshgrid(*[(-1, 1)] * dim, indexing="ij")).reshape(dim, -1).T
    add("square", corners * 500000)                                                        # nrm == 0: no rotation fires
    add("square_345", np.concatenate([s * 100000 * e[k] for k in range(dim) for s in (-1, 1)]).reshape(-1, dim))
    add("rot_cube", _rounded_rotation(corners * 500000, (0.3, 1.1, -0.7)))                 # near-multiple eigenvalue, off-diagonals
    add("rot_cube_small", _rounded_rotation(corners * 3, (0.3, 1.1, -0.7)))
    if dim == 3:
        add("spheroid_oblique", cross(frame, 300000, (0.04, 0.04))[0])                     # a repeated pair, oblique
        add("spheroid_oblate", cross(frame, 300000, (1.0, 0.04))[0])
    # one quantum thick, 2^21 long, oblique
    t = np.linspace(-(1 << 18) + 1, (1 << 18) - 1, 33).astype(np.int64)
    thin = t[:, None] * np.array((4, 3) + pad)
    thin[:, 1] += t & 1
    if dim == 3:
        thin[:, 2] += (t >> 1) & 1
    add("thin_oblique", thin)
    # (the cell is chosen from the float32 difference p - o, whose ulp here is four quanta: 2^21 - 4 is the last offset
    # that the rounding leaves in its cell)
    add("cell_corners", np.where(corners > 0, LIM - 4, -LIM))
    add("far_mean", np.array((LIM - 100, -LIM + 50) + (LIM - 300,) * (dim - 2)) + rng.integers(-40, 40, size=(5, dim)))
    # 64 points within two quanta of each other at the far corner: n Suu and Su Su are 2^54 and differ by a few thousand,
    # so the numerator must be formed in integers (float64 products lose it)
    add("far_tight64", np.array((LIM - 50, -LIM + 50) + (LIM - 50,) * (dim - 2)) + rng.integers(-2, 3, size=(64, dim)))
    # the clamp boundary: lambda_k / lambda_max = eig_ratio (1 -+ 5e-7) (to the 1.2e-7 that the integer sums of
    # 16 long pairs resolve at eig_ratio = 1e-6), oblique
    amax = (LIM - 8) // max(abs(v) for row in frame for v in row)
    for er in sorted({p[1] for p in PARAMS}):
        for side, f in (("below", 1.0 - 5e-7), ("above", 1.0 + 5e-7)):
            if er == 1.0 and side == "above":
                continue
            if dim == 2:
                add(f"clamp_{er:g}_{side}", cross(frame, amax, (er * f,), m=16)[0])
            else:
                add(f"clamp_mid_{er:g}_{side}", cross(frame, amax, (er * f, er * er * 0.01), m=16)[0])
                add(f"clamp_min_{er:g}_{side}", cross(frame, amax, (min(1.0, 30 * er), er * f), m=16)[0])
    add("ill_1e-6_unclamped", cross(frame, amax, (1.001e-6,) * (dim - 1))[0])
    add("ill_1e-6_axes", cross(axes, LIM - 8, (1.001e-6,) * (dim - 1))[0])
    if dim == 3:
        add("graded_oblique", cross(frame, amax, (1e-6, 1e-12))[0])
        add("graded_axes", cross(axes, LIM - 8, (1e-6, 1e-12))[0])
    for n in (3, 5, 17, 200):
        add(f"random{n}", _random_cloud(rng, n, dim))
    add("n_2^20", _big_cell(dim))
    for name, U in cases:
        assert U.min() >= -LIM and U.max() < LIM, name
    return cases


# ---------------------------------------------------------------------------------------------- catalogues
class Catalogue:
    """name, dim, c, cloud float32 [n, dim], blob uint8 (what save_map must give), names {cell key: case name},
    big = the key of a cell with 2^20 points (or None), extra(rng, n) = points inside the grid that avoid that cell."""

    def __init__(self, name, dim, c, cloud, blob, names, big=None):
        self.name, self.dim, self.c, self.cloud, self.blob, self.names, self.big = name, dim, c, cloud, blob, names, big
        self.h, self.cells = R.parse(blob)
        self.ext = [self.h["width"], self.h["height"], self.h["depth"]][:dim]

    def coords(self, pts=None):
        pts = self.cloud if pts is None else pts
        return tuple(np.ascontiguousarray(pts[:, a]) for a in range(self.dim))

    def cell_name(self, k):
        return self.names.get(int(k), f"cell {int(k)}")

    def extent_points(self):
        """indices of the cloud's extreme points: a part of the cloud that holds them has the whole cloud's grid"""
        return np.unique([f(self.cloud[:, a]) for a in range(self.dim) for f in (np.argmin, np.argmax)])


def _lattice(dim):
    c = 0.5
    nside = 8 if dim == 2 else 6
    lo = -0.5 * nside * c
    cases = lattice_cases(dim)
    assert len(cases) <= nside ** dim
    clouds, where = [], []
    for j, (name, U) in enumerate(cases):
        idx = [(j // nside ** a) % nside for a in range(dim)]
        centre = np.array([lo + (i + 0.5) * c for i in idx])
        p = centre[None, :] + U.astype(np.float64) * 2.0 ** -23
        p32 = p.astype(np.float32)
        assert np.array_equal(p32.astype(np.float64), p), name
        clouds.append(p32)
        where.append(idx)
    cloud = np.concatenate(clouds)
    origin, ext = R.grid_geometry(cloud, c)
    off = [int(round((lo - float(origin[a])) / c)) for a in range(dim)]
    ncell = int(np.prod(ext))
    cells = np.zeros(ncell, dtype=R.cell_dtype(dim))
    names, big = {}, None
    pairs = [(a, b) for a in range(dim) for b in range(a, dim)]
    for (name, U), idx in zip(cases, where):
        g = [off[a] + idx[a] for a in range(dim)]
        k = g[0] + ext[0] * (g[1] + (ext[1] * g[2] if dim == 3 else 0))
        names[k] = name
        if len(U) == 1 << 20:
            big = k
        cells["n"][k] = len(U)
        cells["s"][k] = U.sum(axis=0)
        cells["ss"][k] = [int((U[:, a] * U[:, b]).sum()) for a, b in pairs]
    o4 = np.zeros((4, 3), dtype=np.float32)
    if dim == 2:
        k0 = [int(np.rint(float(origin[a]) / c)) for a in range(2)]
        for q, (sx, sy) in enumerate(((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5))):
            o4[q, 0] = np.float32((k0[0] - sx) * c)
            o4[q, 1] = np.float32((k0[1] - sy) * c)
    else:
        o4[0] = origin
    h = dict(magic=R.MAGIC, version=1, dims=dim, ngrid=1, width=ext[0], height=ext[1], depth=ext[2] if dim == 3 else 1,
             cell_bytes=R.cell_dtype(dim).itemsize, cell_size=c, n_cells=ncell, n_points=len(cloud) if dim == 2 else 0,
             origin=o4)
    return Catalogue(f"lattice{dim}", dim, c, cloud, R.pack(h, cells), names, big)


def _far_cloud(rng, dim, centre):
    """A few hundred arbitrary float32 points within ~1.5 m of `centre`: anisotropic blobs, a straight wall (rank-1 cells),
    a floor patch in 3D (rank 2), exact duplicates, a pair and a single point on their own."""
    parts = []
    for _ in range(4):
        scale = rng.uniform(0.002, 0.25, dim)
        p = rng.normal(size=(40, dim)) * scale
        parts.append(_rotate(p, rng) + rng.uniform(-1.2, 1.2, dim))
    wall = np.zeros((60, dim))
    wall[:, 0] = np.linspace(-1.4, 1.4, 60)
    wall[:, 1] = 0.35 * wall[:, 0] + 0.2
    parts.append(wall)
    if dim == 3:
        floor = rng.uniform(-1.0, 1.0, size=(80, 3))
        floor[:, 2] = -0.55
        parts.append(floor)
    p = np.concatenate(parts)
    p = np.concatenate([p, p[rng.integers(0, len(p), 25)], rng.uniform(-1.4, 1.4, size=(12, dim))])
    return (p + np.asarray(centre)).astype(np.float32)


def _rotate(p, rng):
    """p turned by seeded angles (plain sines and cosines: no LAPACK in what decides the committed expectations)."""
    dim = p.shape[1]
    Rm = np.eye(dim)
    for i, j in ((0, 1), (0, 2), (1, 2))[:1 if dim == 2 else 3]:
        t = float(rng.uniform(0, 2 * math.pi))
        G = np.eye(dim)
        G[i, i] = G[j, j] = math.cos(t)
        G[i, j], G[j, i] = -math.sin(t), math.sin(t)
        Rm = G @ Rm
    return p @ Rm.T


def _far(dim):
    out = []
    signs = np.array(np.meshgrid(*[(-1, 1)] * dim, indexing="ij")).reshape(dim, -1).T
    rng = np.random.default_rng(700 + dim)
    for j, sg in enumerate(signs):
        centre = sg * np.array([700.0, 700.0, 40.0][:dim]) + rng.uniform(-0.3, 0.3, dim)
        cloud = _far_cloud(rng, dim, centre)
        blob = R.blob_from_points(cloud, 0.3)[0]
        out.append(Catalogue(f"far{dim}_{j}", dim, 0.3, cloud, blob, {}))
    return out


@functools.lru_cache(maxsize=None)
def catalogues(dim):
    """[the lattice catalogue, the far catalogues...] of one dimension."""
    return [_lattice(dim)] + _far(dim)


def extra_cloud(cat, n, seed=5):
    """n seeded points inside the catalogue's occupied box that avoid a cell with 2^20 points (one more would overflow it):
    what the removal path adds and takes out again."""
    rng = np.random.default_rng(seed)
    lo, hi = cat.cloud.min(axis=0).astype(np.float64), cat.cloud.max(axis=0).astype(np.float64)
    p = rng.uniform(lo, hi, size=(4 * n, cat.dim)).astype(np.float32)
    p = np.clip(p, cat.cloud.min(axis=0), cat.cloud.max(axis=0))
    if cat.big is not None:
        origin = np.asarray(cat.h["origin"], dtype=np.float32)[0, :cat.dim]
        idx = ((p - origin) * np.float32(1.0 / cat.c)).astype(np.int64)
        key = idx[:, 0] + cat.ext[0] * (idx[:, 1] + (cat.ext[1] * idx[:, 2] if cat.dim == 3 else 0))
        p = p[key != cat.big]
    return p[:n]


# ---------------------------------------------------------------------------------------------- the committed expectations
@functools.lru_cache(maxsize=None)
def _golden_file():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def golden(cat, p):
    """The exact records of catalogue `cat` under PARAMS[p], in the dense form of cell_record_ref (dict of arrays over all
    cells), from tests/golden/cell_records.npz - which stores the valid cells only."""
    z = _golden_file()
    assert tuple(z["params"][p]) == tuple(float(v) for v in PARAMS[p])
    dim, ncell = cat.dim, cat.h["n_cells"]
    ns = dim * (dim + 1) // 2
    key = z[f"{cat.name}/{p}/key"]
    out = dict(valid=np.zeros(ncell, bool), mean=np.zeros((ncell, dim)), icov=np.zeros((ncell, ns)), cov=np.zeros((ncell, ns)),
               kappa=np.zeros(ncell))
    out["valid"][key] = True
    for f in ("mean", "icov", "cov", "kappa"):
        out[f][key] = z[f"{cat.name}/{p}/{f}"]
    return out


def golden_arrays(dims=(2, 3)):
    """What the generator writes: {array name: array}.  Needs mpmath."""
    import cell_record_ref as X
    out = {"params": np.array(PARAMS, dtype=np.float64)}
    for dim in dims:
        for cat in catalogues(dim):
            ex = X.exact_cells(cat.blob)
            for p, (mp, er) in enumerate(PARAMS):
                rec = ex.records(mp, er)
                key = np.flatnonzero(rec["valid"]).astype(np.int32)
                out[f"{cat.name}/{p}/key"] = key
                for f in ("mean", "icov", "cov", "kappa"):
                    out[f"{cat.name}/{p}/{f}"] = rec[f][key]
    return out
