"""The seam catalogue: small seeded targets whose validity is a checkerboard, sources whose every point has its image on
a cell seam or one ulp below it (or on the ring, at the grid's edge, far outside, non-finite), poses whose rotation
values keep clear of float32 rounding ties, and the exact expected hits per kernel family (tests/seam_ref.py).

A cell (ix + iy [+ iz]) even holds min_points + 2 points near the corners of its inner box (spread about 0.4 c, all at
least 0.15 c inside), an odd cell is empty: one misplaced source point flips a hit.  With `exact=True` a valid cell holds
exactly min_points points, one of them on the cell's own lower seam or one ulp below it (then it belongs to the empty
neighbour): misbinning that target point changes the cell's validity.

Everything is deterministic: the only random choices are seeded subsamples.
"""
import functools
import math
from dataclasses import dataclass, field

import numpy as np

import seam_ref as S
from oracle import ndt2d as o2
from oracle import ndt3d as o3

F32 = np.float32
PI = math.pi
MIN_POINTS = {2: 3, 3: 5}
SIDE = {2: 12, 3: 8}
SCORE_TOL_REL, SCORE_TOL_ABS = 1e-4, 1e-3        # tests/test_gpu_score_poses.py, test_score_volume_matches_the_oracle
SCORE_PACK = 16                                  # points per source of the score-only families (see smallest_term)

# (cell size, bounding-box minimum per axis)
TARGETS_2D = [(0.1, 0.0), (0.1, -7.3), (0.1, 800.0), (0.1, -800.0), (0.3, 0.0), (0.3, -3.1), (0.3, 800.0), (0.3, -800.0),
              (0.75, 0.0), (0.75, -7.3), (0.75, 800.0), (0.75, -800.0), (0.5, -3.1), (0.5, 800.0), (1.0, 0.0), (1.0, -800.0),
              (2.0, -7.3), (2.0, 800.0)]
TARGETS_3D = [(0.5, 0.0), (0.5, 300.0), (0.75, -3.1), (0.75, -300.0), (1.0, 0.0), (1.0, 300.0), (2.0, -7.3), (2.0, -300.0)]

f32 = lambda v: float(F32(v))
POSES_2D = {
    "identity": (0.0, 0.0, 0.0),
    "shift": (0.25, -0.5, 0.0),
    "shift_inexact_cell": (f32(0.1), f32(-0.3), 0.0),
    "quarter": (0.5, 0.25, PI / 2),
    "minus_quarter": (-0.25, 0.5, -PI / 2),
    "half": (0.125, -0.125, PI),
    "generic_a": (0.37, -0.21, 0.3),
    "generic_b": (-1.3, 0.8, -1.1),
    "generic_c": (0.05, 2.2, 2.5),
    "beyond_pi": (0.2, -0.1, 7.0),
    "below_minus_pi": (-0.4, 0.3, -9.5),
}
POSES_3D = {
    "identity": (0.0,) * 6,
    "shift": (0.25, -0.5, 0.125, 0.0, 0.0, 0.0),
    "yaw_quarter": (0.5, 0.25, -0.25, 0.0, 0.0, PI / 2),
    "yaw_minus_quarter": (-0.25, 0.5, 0.0, 0.0, 0.0, -PI / 2),
    "yaw_half": (0.125, -0.125, 0.25, 0.0, 0.0, PI),
    "generic_a": (0.37, -0.21, 0.1, 0.02, -0.03, 0.4),
    "generic_b": (-1.3, 0.8, 0.3, -0.05, 0.04, -2.0),
    "steep": (0.3, -0.2, 0.1, 0.9, -1.2, 0.7),                   # steep roll and pitch, as tests/tilted_cases.py
    "beyond_pi": (0.2, -0.1, 0.05, 0.1, -0.2, 7.0),
}
POSES = {2: POSES_2D, 3: POSES_3D}
# the poses a target is met at: identity and one translation everywhere, the rotations in turn
ROTATIONS = {2: ["quarter", "minus_quarter", "half", "generic_a", "generic_b", "generic_c", "beyond_pi", "below_minus_pi"],
             3: ["yaw_quarter", "yaw_minus_quarter", "yaw_half", "generic_a", "generic_b", "steep", "beyond_pi"]}
FAR = [1e6, -1e6, 3e9, -3e9, 1e15, -1e15, 1e30, -1e30]


@dataclass
class Target:
    name: str
    dim: int
    c: float
    base: float
    coords: tuple                 # float32 arrays
    kw: dict                      # matcher options
    grid: object                  # oracle grid (grid 0)
    exact: bool = False
    stretch: int = 0
    seams: list = field(default_factory=list)     # per axis: float32 seam values k = 0 .. extent

    @property
    def ext(self):
        return (self.grid.W, self.grid.H) if self.dim == 2 else tuple(self.grid.dims)

    @property
    def origin(self):
        return (self.grid.ox, self.grid.oy) if self.dim == 2 else tuple(self.grid.o)

    @property
    def geom(self):
        g = self.grid
        return (g.ox, g.oy, g.inv_c, g.W, g.H) if self.dim == 2 else (g.o, g.inv_c, tuple(g.dims))


def _params(dim, c, **more):
    return dict(cell_size=c, min_points=MIN_POINTS[dim], eig_ratio=1e-2, **more)


def _oracle_params(dim, kw, overlap=1):
    if dim == 2:
        return o2.NdtParams(cell_size=kw["cell_size"], min_points=kw["min_points"], eig_ratio=kw["eig_ratio"], overlap=overlap)
    return o3.Ndt3Params(cell_size=kw["cell_size"], min_points=kw["min_points"], eig_ratio=kw["eig_ratio"])


def target_name(dim, c, base, exact=False, stretch=0):
    return f"{dim}d c={c} min={base}" + (" exact" if exact else "") + (f" stretched to {stretch}" if stretch else "")


@functools.lru_cache(maxsize=None)
def target(dim: int, c: float, base: float, exact: bool = False, stretch: int = 0) -> Target:
    """The checkerboard target.  stretch = n: one more lone point n cells beyond the minimum on every axis, so that the
    grid outgrows the batch kernels' on-chip tables while the point count stays in the hundreds."""
    side, mp = SIDE[dim], MIN_POINTS[dim]
    lo = math.floor(base / c) * c               # on the grid's own lattice: an intended cell is one cell of the grid
    rng = np.random.default_rng([dim, int(c * 1000), int(abs(base) * 10), int(base < 0), int(exact)])
    pts = []
    corners = np.array(list(np.ndindex(*(2,) * dim)), np.float64)
    lows = {}                                 # cell -> index of the point to be put on the cell's own lower seam
    for cell in np.ndindex(*(side,) * dim):
        if sum(cell) % 2:
            continue
        # the corners of the inner box [0.15, 0.85]^dim in a seeded order (2D: and the centre), a little jitter: a spread of
        # about 0.35 c on every axis and a well-conditioned covariance, so a point on a seam still scores about 0.4
        n = mp if exact else mp + 2
        u = 0.15 + 0.7 * corners[rng.permutation(len(corners))]
        if dim == 2 and not exact:
            u = np.concatenate([u, [[0.5, 0.5]]])
        u = u[:n] + rng.uniform(-0.02, 0.02, (n, dim))
        lows[cell] = len(pts)
        pts.extend((lo + (np.array(cell) + u[k]) * c) for k in range(n))
    P = np.array(pts, np.float64).astype(F32)
    if stretch:
        P = np.concatenate([P, np.full((1, dim), lo + (stretch - 0.5) * c, F32)])
    kw = _params(dim, c)
    prm = _oracle_params(dim, kw)
    cols = tuple(np.ascontiguousarray(P[:, a]) for a in range(dim))
    geometry = (lambda cc: o2.grid_geometry(cc[0], cc[1], c)) if dim == 2 else (lambda cc: o3.grid_geometry3(np.stack(cc, 1), c))
    if exact:
        # the geometry does not move when a point moves onto its cell's lower seam (the minimum stays in its cell ...)
        geo = geometry(cols)
        if dim == 2:
            org, inv_c = (geo[0], geo[1]), geo[2]
        else:
            org, inv_c = tuple(geo[0]), geo[1]
        flat = lambda ge: [float(v) for part in ge for v in np.ravel(part)]
        for j, (cell, first) in enumerate(lows.items()):
            if min(cell) == 0:
                continue                                               # ... because cells on the low border keep theirs
            axis = j % dim
            k = int(S.cell_index32(P[first, axis], org[axis], inv_c))
            s = S.seam(org[axis], inv_c, k)
            P[first, axis] = s if (j // dim) % 2 == 0 else S.below(s)
        cols = tuple(np.ascontiguousarray(P[:, a]) for a in range(dim))
        assert flat(geometry(cols)) == flat(geo)
    grid = o2.build_grid(cols[0], cols[1], prm) if dim == 2 else o3.build_grid3(*cols, prm)
    t = Target(target_name(dim, c, base, exact, stretch), dim, c, base, cols, kw, grid, exact, stretch)
    for a in range(dim):
        t.seams.append(np.array([S.seam(t.origin[a], grid.inv_c, k) for k in range(t.ext[a] + 1)], F32))
    return t


def overlap_grids(t: Target):
    """The four grids of overlap_grids = 4 on a 2D target (ALGORITHM 2.7)."""
    return o2.build_grids(t.coords[0], t.coords[1], _oracle_params(2, t.kw, overlap=4))


# ------------------------------------------------------------------------------------------------ wanted images
def _seam_values(t: Target, axis: int, side: int):
    """Per seam of the first `side + 3` cells of one axis and of the last two: (value, seam index k, on: 1 on the seam, 0
    below it).  k = 0 and k = extent come with one more step outward: f in (-1, 0) twice, and one ulp past f == extent."""
    ext = t.ext[axis]
    ks = sorted(set(range(0, min(side + 3, ext) + 1)) | {ext - 1, ext})
    out = []
    for k in ks:
        s = t.seams[axis][k]
        out += [(S.below(s), k, 0), (s, k, 1)]
        if k == 0:
            out.append((S.below(S.below(s)), k, 0))
        if k == ext:
            out.append((S.above(s), k, 1))
    return out


def _mids(t: Target, axis: int, side: int):
    s = t.seams[axis].astype(np.float64)
    n = min(side + 2, t.ext[axis])
    return (0.5 * (s[:n] + s[1:n + 1])).astype(F32)


@functools.lru_cache(maxsize=None)
def wanted(dim, c, base, stretch=0):
    """The images the sources aim at: (Q [n, dim] float32, want [n, dim] bool: the axis must be met to the bit,
    seam [n, dim] int: the seam index on a wanted axis, -1 elsewhere, on [n, dim]: 1 on the seam, 0 below)."""
    t = target(dim, c, base, False, stretch)
    side = SIDE[dim]
    rng = np.random.default_rng([7, dim, int(c * 1000), int(abs(base) * 10)])
    vals = [_seam_values(t, a, side) for a in range(dim)]
    mids = [_mids(t, a, side) for a in range(dim)]
    rows = []
    if dim == 2:
        for a in range(2):                                                    # one axis on a seam, the other mid-cell
            for v, k, on in vals[a]:
                for m in mids[1 - a]:
                    q, w = [0, 0], [False, False]
                    q[a], q[1 - a], w[a] = v, m, True
                    rows.append((q, w, [k if i == a else -1 for i in range(2)], [on if i == a else 0 for i in range(2)]))
        for v0, k0, on0 in vals[0]:                                           # corners
            for v1, k1, on1 in vals[1]:
                rows.append(([v0, v1], [True, True], [k0, k1], [on0, on1]))
    else:
        for a in range(3):
            b, d = [i for i in range(3) if i != a]
            cells = [(i, j) for i in range(len(mids[b])) for j in range(len(mids[d]))]
            for v, k, on in vals[a]:
                for n_ in rng.choice(len(cells), 12, replace=False):
                    i, j = cells[n_]
                    q, w = [0, 0, 0], [False] * 3
                    q[a], q[b], q[d], w[a] = v, mids[b][i], mids[d][j], True
                    rows.append((q, w, [k if x == a else -1 for x in range(3)], [on if x == a else 0 for x in range(3)]))
        for _ in range(360):                                                  # edges: two axes on seams
            a = int(rng.integers(0, 3))
            b, d = [i for i in range(3) if i != a]
            (vb, kb, ob), (vd, kd, od) = vals[b][rng.integers(len(vals[b]))], vals[d][rng.integers(len(vals[d]))]
            q, w, k, on = [0, 0, 0], [True] * 3, [-1] * 3, [0] * 3
            q[a], w[a] = mids[a][rng.integers(len(mids[a]))], False
            q[b], q[d], k[b], k[d], on[b], on[d] = vb, vd, kb, kd, ob, od
            rows.append((q, w, k, on))
        for _ in range(360):                                                  # corners: all three
            pick = [vals[a][rng.integers(len(vals[a]))] for a in range(3)]
            rows.append(([p[0] for p in pick], [True] * 3, [p[1] for p in pick], [p[2] for p in pick]))
    Q = np.array([r[0] for r in rows], F32)
    return Q, np.array([r[1] for r in rows], bool), np.array([r[2] for r in rows], int), np.array([r[3] for r in rows], int)


# ------------------------------------------------------------------------------------------------ sources at a pose
def image(dim, coords, pose, family="chain"):
    if dim == 2:
        return S.image2d(coords[0], coords[1], pose)
    return (S.image3d_batch if family == "batch3" else S.image3d)(*coords, pose)


def _inverse(dim, Q, pose):
    if dim == 2:
        th = o2.wrap_angle(float(pose[2]))
        R = np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
    else:
        R = np.array(S.rot3d_entries(*pose[3:6])).reshape(3, 3)
    t = np.array([float(F32(v)) for v in pose[:dim]])
    return (Q.astype(np.float64) - t) @ R                                   # R^T (q - t), row vectors


@dataclass
class Source:
    coords: tuple                 # float32 arrays, the seam points first, then the specials
    seam: np.ndarray              # [n, dim] seam index per axis the point was placed on (-1: none)
    on: np.ndarray                # [n, dim] 1: on the seam, 0: below it
    n_seam_points: int


@functools.lru_cache(maxsize=None)
def source(dim, c, base, pose_name, stretch=0, limit=0) -> Source:
    """Source points whose exact image (the chain form) at the pose lies on the wanted seams: the pose is inverted
    approximately, neighbouring float32 source values are walked, and those whose exact image meets the wanted axes to the
    bit are kept.  Then far-outside and non-finite points.  limit > 0: a seeded subsample of the wanted images first."""
    t = target(dim, c, base, False, stretch)
    pose = POSES[dim][pose_name]
    Q, want, seam, on = wanted(dim, c, base, stretch)
    rotated = any(float(v) != 0.0 for v in pose[dim:])
    if limit == 0 and rotated:
        limit = 400 if dim == 2 else 240
    if limit and limit < len(Q):
        pick = np.sort(np.random.default_rng([11, len(Q)]).choice(len(Q), limit, replace=False))
        Q, want, seam, on = Q[pick], want[pick], seam[pick], on[pick]
    s0 = _inverse(dim, Q, pose).astype(F32)
    reach = (12 if dim == 2 else 5) if rotated else (3 if dim == 2 else 2)
    steps = np.arange(-reach, reach + 1)
    offs = np.array(np.meshgrid(*[steps] * dim, indexing="ij")).reshape(dim, -1).T          # [m, dim]
    offs = offs[np.argsort(np.abs(offs).sum(axis=1), kind="stable")]                        # nearest first
    cand = (s0[:, None, :].astype(np.float64) + offs[None] * np.spacing(np.abs(s0))[:, None, :].astype(np.float64)).astype(F32)
    img = image(dim, tuple(cand[..., a] for a in range(dim)), pose)
    ok = np.ones(cand.shape[:2], bool)
    for a in range(dim):
        free_ok = np.abs(img[a].astype(np.float64) - Q[:, None, a].astype(np.float64)) < 0.25 * c
        ok &= np.where(want[:, None, a], img[a] == Q[:, None, a], free_ok)
    found = ok.any(axis=1)
    first = ok.argmax(axis=1)
    P = cand[np.arange(len(Q)), first][found]
    seam, on = np.where(want, seam, -1)[found], on[found]
    n_seam = len(P)
    # specials: far outside and non-finite, per coordinate, the others mid-grid (source frame: at these magnitudes the pose
    # does not bring them back)
    mid = _inverse(dim, np.array([[0.5 * (float(t.seams[a][0]) + float(t.seams[a][-1])) for a in range(dim)]], F32), pose)[0]
    special = []
    for a in range(dim):
        for v in FAR + [np.nan, np.inf, -np.inf]:
            p = mid.copy()
            p[a] = v
            special.append(p)
    special.append(np.full(dim, np.nan))
    with np.errstate(over="ignore"):
        P = np.concatenate([P, np.array(special).astype(F32)])
    pad = -np.ones((len(special), dim), int)
    return Source(tuple(np.ascontiguousarray(P[:, a]) for a in range(dim)), np.concatenate([seam, pad]),
                  np.concatenate([on, 0 * pad]), n_seam)


def packed(src: Source, n: int, seed: int = 0):
    """n points of the source (seeded order; the source repeated where it is shorter): tails, waves, both scan kernels."""
    m = len(src.coords[0])
    order = np.random.default_rng([13, seed, m]).permutation(m)
    idx = np.resize(order, n)
    return tuple(np.ascontiguousarray(cc[idx]) for cc in src.coords), idx


# ------------------------------------------------------------------------------------------------ expected values
NB7 = ((0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))      # ALGORITHM 2.25


def point_hits(t: Target, coords, pose, family="chain", overlap=1, neighbourhood=1, image_fn=None, index_rule=None,
               neighbours_by_key=False):
    """Hits per point (an integer: grids, or voxels of the neighbourhood, whose record the point reads) and the keys of
    grid 0 / the own voxel (-1 outside).  image_fn / index_rule: the mutants of tests/test_seam_ref.py."""
    dim = t.dim
    fin = S.finite_points(*coords)
    img = image_fn(*coords, pose) if image_fn else image(dim, coords, pose, family)
    if dim == 2:
        grids = overlap_grids(t) if overlap == 4 else [t.grid]
        hits = np.zeros(len(fin), int)
        key0 = None
        for g in grids:
            if index_rule:
                ix, inx = S.index_mutant(index_rule, img[0], g.ox, g.inv_c, t.c, g.W)
                iy, iny = S.index_mutant(index_rule, img[1], g.oy, g.inv_c, t.c, g.H)
                key, inside = iy * g.W + ix, inx & iny
            else:
                key, inside = S.keys2d(img[0], img[1], (g.ox, g.oy, g.inv_c, g.W, g.H))
            inside = inside & fin
            hits += inside & g.valid[np.where(inside, key, 0)]
            if key0 is None:
                key0 = np.where(inside, key, -1)
        return hits, key0
    g = t.grid
    if index_rule:
        parts = [S.index_mutant(index_rule, img[a], g.o[a], g.inv_c, t.c, g.dims[a]) for a in range(3)]
        idx = np.stack([p[0] for p in parts], axis=1)
        inside = parts[0][1] & parts[1][1] & parts[2][1]
        key = (idx[:, 2] * g.dims[1] + idx[:, 1]) * g.dims[0] + idx[:, 0]
    else:
        key, inside, idx = S.keys3d(*img, t.geom)
    inside = inside & fin
    hits = np.zeros(len(fin), int)
    dims = np.array(g.dims)
    for d in NB7[:neighbourhood]:
        j = idx + np.array(d)
        k = (j[:, 2] * dims[1] + j[:, 1]) * dims[0] + j[:, 0]
        if neighbours_by_key:                                                # the mutant: key - 1 from ix = 0 is the last
            ok = inside & (k >= 0) & (k < len(g.valid))                      # voxel of the row before
        else:
            ok = inside & np.all((j >= 0) & (j < dims), axis=1)              # by index, never by key arithmetic
        hits += ok & g.valid[np.where(ok, k, 0)]
    return hits, np.where(inside, key, -1)


def _grid3_on_geometry(P32, o, inv_c, dims, prm):
    """oracle.ndt3d.build_grid3 on a given geometry (a reserved grid): a point is binned where 0 <= f < extent on every
    axis, ring voxels included (ALGORITHM 2.17: 3D has no empty-ring contract)."""
    key, inside = o3.cell_keys3(P32, o, inv_c, dims)
    assert inside.all()
    nc = int(np.prod(dims))
    P = P32.astype(np.float64)
    count = np.bincount(key, minlength=nc).astype(np.int64)
    nz = np.maximum(count, 1)[:, None]
    mean = np.stack([np.bincount(key, weights=P[:, a], minlength=nc) for a in range(3)], axis=1) / nz
    d = P - mean[key]
    mean = mean + np.stack([np.bincount(key, weights=d[:, a], minlength=nc) for a in range(3)], axis=1) / nz
    d = P - mean[key]
    M2 = np.stack([np.bincount(key, weights=d[:, i] * d[:, j], minlength=nc)
                   for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], axis=1)
    cand = np.nonzero(count >= max(prm.min_points, 2))[0]
    valid, icov = np.zeros(nc, bool), np.zeros((nc, 6))
    ok, ic = o3.finalise_cells3(count[cand], M2[cand], prm)
    valid[cand], icov[cand] = ok, ic
    mean[~valid] = 0.0
    return o3.Grid3D(o, inv_c, tuple(dims), count, mean, icov, valid, int(valid.sum()))


RING_NAME = "3d c=1.0 min=0.0 ring voxels filled @ identity"


@functools.lru_cache(maxsize=None)
def ring_case():
    """A 3D grid whose outermost voxels hold points: the checkerboard target's geometry as a reserved grid, its points,
    and clusters in the first and the last voxel of every x row of the middle layers.  Sources sit on the seams of those
    voxels.  Here a face neighbour taken by key arithmetic (key + 1 from the last voxel of a row is the first voxel of
    the next) finds a valid voxel where the neighbour by index does not exist.
    -> (Target, (lo, hi) of reserve_target, source coords)"""
    t0 = target(3, 1.0, 0.0)
    g0, c = t0.grid, 1.0
    W, H, D = g0.dims
    rng = np.random.default_rng(23)
    corners = np.array(list(np.ndindex(2, 2, 2)), np.float64)
    extra, src = [], []
    for ix in (0, W - 1):
        for iy in range(1, H - 1):
            for iz in range(2, D - 2):
                cell = np.array([ix, iy, iz])
                u = 0.15 + 0.7 * corners[rng.permutation(8)][:7] + rng.uniform(-0.02, 0.02, (7, 3))
                extra.extend(g0.o.astype(np.float64) + (cell + u[k]) * c for k in range(7))
                mid = [0.5 * (float(t0.seams[a][cell[a]]) + float(t0.seams[a][cell[a] + 1])) for a in range(3)]
                for k in (ix, ix + 1):
                    for x in (S.below(t0.seams[0][k]), t0.seams[0][k]):
                        src.append([x, mid[1], mid[2]])
    P = np.concatenate([np.stack(t0.coords, axis=1), np.array(extra).astype(F32)])
    lo = tuple(float(v.min()) for v in t0.coords)
    hi = tuple(float(v.max()) for v in t0.coords)
    grid = _grid3_on_geometry(P, g0.o, g0.inv_c, g0.dims, _oracle_params(3, t0.kw))
    t = Target(RING_NAME, 3, c, 0.0, tuple(np.ascontiguousarray(P[:, a]) for a in range(3)), t0.kw, grid, seams=t0.seams)
    Q = np.array(src, F32)
    return t, (lo, hi), tuple(np.ascontiguousarray(Q[:, a]) for a in range(3))


def n_hit(t, coords, pose, **how) -> int:
    return int(point_hits(t, coords, pose, **how)[0].sum())


def score_terms(t: Target, coords, pose, family="chain"):
    """The float64 score term d1 exp(-d2/2 m) of every point that hits (one grid, own voxel; d1 = d2 = 1), from the
    reference keys, the float32 image and the oracle's records rounded to float32 as the device stores them (the
    oracle's mirror does the same); terms and sums in float64; 0 for a miss."""
    hits, key = point_hits(t, coords, pose, family)
    img = np.stack([np.asarray(v, np.float64) for v in image(t.dim, coords, pose, family)], axis=1)
    g = t.grid
    out = np.zeros(len(hits))
    h = hits > 0
    mean, icov = (r.astype(np.float64) for r in g.records32())          # a record is stored as float32 (ALGORITHM 2.3)
    q = img[h] - mean[key[h]]
    ic = icov[key[h]]
    if t.dim == 2:
        m = ic[:, 0] * q[:, 0] ** 2 + 2 * ic[:, 1] * q[:, 0] * q[:, 1] + ic[:, 2] * q[:, 1] ** 2
    else:
        m = (ic[:, 0] * q[:, 0] ** 2 + ic[:, 3] * q[:, 1] ** 2 + ic[:, 5] * q[:, 2] ** 2
             + 2 * (ic[:, 1] * q[:, 0] * q[:, 1] + ic[:, 2] * q[:, 0] * q[:, 2] + ic[:, 4] * q[:, 1] * q[:, 2]))
    out[h] = np.exp(-0.5 * m)
    return out


def score_tolerance(score: float) -> float:
    return SCORE_TOL_REL * abs(score) + SCORE_TOL_ABS


def score_packs(t: Target, src: Source, pose, family="chain", n_packs=6):
    """Sources of SCORE_PACK points for the families that return a score only: points on one seam (the other axes
    mid-cell), where a term is large against the tolerance.  -> list of (coords, exact score, smallest term)."""
    single = np.flatnonzero((src.seam >= 0).sum(axis=1) == 1)
    rng = np.random.default_rng([17, len(single)])
    out = []
    for _ in range(n_packs):
        idx = rng.choice(single, min(SCORE_PACK, len(single)), replace=False)
        cc = tuple(np.ascontiguousarray(v[idx]) for v in src.coords)
        terms = score_terms(t, cc, pose, family)
        out.append((cc, float(terms.sum()), float(terms[terms > 0].min()) if (terms > 0).any() else math.inf))
    return out


# ------------------------------------------------------------------------------------------------ the catalogue
def entries(dim):
    """(cell size, minimum, pose name) of every catalogue entry: each target at the identity, at a translation and at two
    of the rotations, taken in turn so that every rotation meets near, negative and far targets."""
    rots = ROTATIONS[dim]
    out = []
    for i, (c, base) in enumerate(TARGETS_2D if dim == 2 else TARGETS_3D):
        shift = "shift_inexact_cell" if (dim == 2 and i % 2) else "shift"
        for name in ["identity", shift, rots[(2 * i) % len(rots)], rots[(2 * i + 1) % len(rots)]]:
            out.append((c, base, name))
    return out


def entry_name(dim, c, base, pose_name):
    return f"{target_name(dim, c, base)} @ {pose_name}"
