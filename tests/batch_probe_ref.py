"""One-point probes of the per-cell records, for the paths that have no read-back of their records: the grid build inside
k_batch / k_batch3 (tests/test_gpu_batch_records.py).  CPU, numpy only.

THE IDEA.  With fixed_iterations = 1 a result row holds H, g, score and n_hit of the evaluation at the start pose,
whatever the status.  A pair whose source is ONE point inside ONE chosen cell, at the identity pose, therefore reads that
cell's valid bit exactly (n_hit) and its mean and Sigma^-1 through a single term: no summation order.

PROBES (probes(cat, p), for a catalogue of tests/cell_record_cases.py and PARAMS[p]; the records are the exact ones of
tests/golden/cell_records.npz).  Per valid cell one probe  mu + s L z  for each direction z of DIRECTIONS (the axes and
one oblique direction: 3 in 2D, 4 in 3D), L L^T the clamped Sigma, s the first of +1, -1, +1/2, -1/2, +1/4, -1/4 whose
probe, rounded to float32, differs from the rounded mean and lies at least 8 ulp32 (of each coordinate) inside the
cell's faces (float64 centres of cell_record_ref.centres -+ c / 2).  A cell without any such probe gets the rounded mean
itself where that is 8 ulp inside.  At most MAX_UNPLACED probes per (catalogue, parameter set) may stay unplaced and every
valid cell keeps at least one (asserted here; the unplaced ones are at eig_ratio 1e-6 on the far catalogues, where a
one-sigma step along the clamped direction is below the float32 spacing at 700 m).
Probes that must miss, one per cell at the float32 centre: every occupied but invalid cell, every empty interior cell
of a lattice catalogue, 32 seeded empty interior cells of a far catalogue, the corner cells of the guard ring, and one
point 3 cells outside the grid.
Cells are named by their integer coordinates and their centre, never by key: the stretched targets of the GPU file change W.

REFERENCE TERMS (terms(dim, pt, mean, icov, mode)).  docs/ALGORITHM.md 2.4 / 2.6 for one image point and one record at
the identity pose, in float64, both Hessian forms; the input is the exact record, nothing read from a device.

TOLERANCE of a device term against that reference (tolerance()), two parts.
  Storage: every entry of Sigma^-1 moved by the bound check_records holds the stored record to (matrix_tolerance), one
    entry at a time and in either direction; the absolute changes of the output, added up, plus the interaction of every
    two entries (what moving both changes beyond the two separate moves: second order, and what is left where the first
    order cancels).
    The mean is not moved: it is taken as the float32 it must be stored as.  mean_tolerance is half an ulp32 plus a
    float64 part of 1e-11 m, so the stored mean is the exact mean rounded to float32 - unless the exact mean lies within
    the float64 part of a rounding tie (two points one ulp32 apart: the far catalogues have such cells), where it is one
    of the two neighbours and a device row has to meet the reference at one of them (Reference.alt).  Moving the mean
    by the whole of mean_tolerance instead, entry by entry, asks less wherever the response is linear and is no bound
    where it is not: at 700 m half an ulp32 is a sigma of a thin cell and more, and the exact record rounded to float32
    itself came out 3.2 times beyond that sum (test_correct_records_stored_as_float32_pass_every_probe is the control).
  Arithmetic:  C_PROBE eps32 A.  A is the running-error scale of the term: the same expression carried through with
    absolute values, one rounding of size |result| charged per operation (per sum, per product, two for the exponential
    and two for its scaled argument) and propagated to the output by the usual first-order rules; operations that are
    exact in any binary arithmetic (a zero summand, a factor 0 or +-1: the Jacobian of the identity pose) are charged
    nothing, a product and the score 2^-126 on top (float32 flushes what is smaller).  It grows by itself where
    q' Sigma^-1 q cancels.  A float32 evaluation in any order of these operations, fused or not, has an error of at most
    (eps32 / 2) A  to first order, so C_PROBE = 1 leaves a factor of two.
C_PROBE is measured, by the rule of tests/step_replay.py and C_RECORD: the oracle's float32 mirror (evaluate /
evaluate3 with mirror32=True) on a one-cell grid holding the exact record rounded to float32, against these terms at the
same rounded record, over every probe of every catalogue and parameter set and both Hessian forms, in units of eps32 A:

    MEASURED_UNITS[2] = 5.1e-10   (Newton H[0][1] of the probe along +y of cell (3, 5) of far2_0, min_points 2,
                                   eig_ratio 1e-3)
    MEASURED_UNITS[3] = 1.0e-09   (Gauss-Newton H[5][0] of the probe along +x of cell (3, 2, 7) of far3_5, min_points 6,
                                   eig_ratio 0.1)
    At the identity pose the mirror's transform and Jacobian are exact and its terms are float64 sums of float32
    inputs: what is measured is float64 rounding (eps64 / eps32 = 1.9e-9 per rounding), not float32 arithmetic.
    C_PROBE[dim] = 8 x that, rounded up to an integer = 1 and 1

The 3D batch sums in the map frame (accumulate_point3_map: P = sum w C Y, S = sum w Y' C Y, n = sum w y x v, contracted
with the rotation axes in float64).  At the identity pose the axes are the unit vectors, the contraction moves entries
without arithmetic, and the per-point products are those of the Jacobian form in another order; the measurement's factor
8 and the factor two above are what absorb the different order.  tests/test_batch_probe_ref.py checks the measurement
(test_mirror_error_is_an_eighth_of_the_tolerance) and that the probes catch the mutants of cell_record_ref."""
import functools
import math

import numpy as np

import cell_record_cases as K
import cell_record_ref as X
import map_coarsen_ref as R

EPS32 = 2.0 ** -23
MEASURED_UNITS = {2: 5.1e-10, 3: 1.0e-09}
C_PROBE = {2: 1.0, 3: 1.0}
MAX_UNPLACED = 2
INSIDE_ULPS = 8
STEPS = (1.0, -1.0, 0.5, -0.5, 0.25, -0.25)
DIRECTIONS = {2: ((1.0, 0.0), (0.0, 1.0), (math.sqrt(0.5), math.sqrt(0.5))),
              3: ((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0), (math.sqrt(1 / 3),) * 3)}
NPOSE = {2: 3, 3: 6}
N_EMPTY_FAR = 32


def nout(dim):
    """entries of a term vector: H (row-major, full), g, score"""
    return NPOSE[dim] ** 2 + NPOSE[dim] + 1


def out_name(dim, j):
    n = NPOSE[dim]
    return f"H[{j // n}][{j % n}]" if j < n * n else f"g[{j - n * n}]" if j < n * n + n else "score"


# ---------------------------------------------------------------------------------------------- geometry
def cell_key(idx, ext):
    """per-axis indices [n, dim] -> cell number in a grid of extents ext (x fastest)"""
    idx = np.asarray(idx, dtype=np.int64)
    key = idx[:, 0] + ext[0] * idx[:, 1]
    return key + ext[0] * ext[1] * idx[:, 2] if len(ext) == 3 else key


def _inside(pt32, ctr, c):
    """every coordinate of the float32 points at least INSIDE_ULPS ulp32 inside the faces ctr -+ c / 2"""
    p = pt32.astype(np.float64)
    margin = INSIDE_ULPS * X.ulp32(p)
    return np.all((p - margin >= ctr - 0.5 * c) & (p + margin <= ctr + 0.5 * c), axis=-1)


def _cholesky(cov_rows, dim):
    """L with L L^T = the symmetric matrices stored as rows (xx xy yy | xx xy xz yy yz zz), lower triangular;
    a pivot that rounding made negative counts as zero."""
    n = len(cov_rows)
    S = np.zeros((n, dim, dim))
    for p, (a, b) in enumerate(X.PAIRS[dim]):
        S[:, a, b] = S[:, b, a] = cov_rows[:, p]
    L = np.zeros((n, dim, dim))
    for j in range(dim):
        d = S[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
        L[:, j, j] = np.sqrt(np.maximum(d, 0.0))
        safe = np.where(L[:, j, j] > 0.0, L[:, j, j], 1.0)
        for i in range(j + 1, dim):
            L[:, i, j] = np.where(L[:, j, j] > 0.0, (S[:, i, j] - (L[:, i, :j] * L[:, j, :j]).sum(axis=1)) / safe, 0.0)
    return L


@functools.lru_cache(maxsize=None)
def _by_name(dim):
    return {c.name: c for c in K.catalogues(dim)}


def catalogue(name):
    return _by_name(int(name[-1]) if name.startswith("lattice") else int(name[3]))[name]


@functools.lru_cache(maxsize=None)
def _probes(name, p):
    cat = catalogue(name)
    dim, c, ext = cat.dim, cat.c, cat.ext
    exact = K.golden(cat, p)
    ncell = cat.h["n_cells"]
    idx_all = X.cell_index(np.arange(ncell), ext)
    pts, cells, hit, kind = [], [], [], []
    # ---- valid cells: mu + s L z
    vk = np.flatnonzero(exact["valid"])
    ctr = X.centres(cat.h, vk)
    mean = exact["mean"][vk]
    mean32 = mean.astype(np.float32)
    L = _cholesky(exact["cov"][vk], dim)
    unplaced, per_cell = [], np.zeros(len(vk), int)
    for d, z in enumerate(DIRECTIONS[dim]):
        step = L @ np.array(z)
        done = np.zeros(len(vk), bool)
        for s in STEPS:
            cand = (mean + s * step).astype(np.float32)
            ok = ~done & np.any(cand != mean32, axis=1) & _inside(cand, ctr, c)
            for j in np.flatnonzero(ok):
                pts.append(cand[j]); cells.append(idx_all[vk[j]]); hit.append(True); kind.append(f"dir{d} s={s:g}")
            done |= ok
        per_cell += done
        unplaced += [(tuple(idx_all[vk[j]]), d) for j in np.flatnonzero(~done)]
    fallback = (per_cell == 0) & _inside(mean32, ctr, c)
    for j in np.flatnonzero(fallback):
        pts.append(mean32[j]); cells.append(idx_all[vk[j]]); hit.append(True); kind.append("mean")
    per_cell += fallback
    assert len(unplaced) <= MAX_UNPLACED, (name, p, unplaced)
    assert per_cell.min(initial=1) >= 1, (name, p, [tuple(idx_all[vk[j]]) for j in np.flatnonzero(per_cell == 0)])
    n_valid_probes = len(pts)
    # ---- cells that must miss, at their float32 centre
    n = cat.cells["n"][:ncell].astype(np.int64)
    interior = np.all((idx_all >= 1) & (idx_all <= np.array(ext) - 2), axis=1)
    empty = np.flatnonzero(interior & (n == 0))
    if not name.startswith("lattice"):
        empty = np.sort(np.random.default_rng(4242 + p).permutation(empty)[:N_EMPTY_FAR])
    corner = np.flatnonzero(np.all((idx_all == 0) | (idx_all == np.array(ext) - 1), axis=1))
    for what, ks in (("invalid", np.flatnonzero((n > 0) & ~exact["valid"])), ("empty", empty), ("corner", corner)):
        ctr = X.centres(cat.h, ks)
        c32 = ctr.astype(np.float32)
        ok = _inside(c32, ctr, c)
        assert ok.all(), (name, p, what)
        for j in range(len(ks)):
            pts.append(c32[j]); cells.append(idx_all[ks[j]]); hit.append(False); kind.append(what)
    origin = np.asarray(cat.h["origin"], dtype=np.float32)[0, :dim].astype(np.float64)
    pts.append((origin - 2.5 * c).astype(np.float32)); cells.append(np.full(dim, -3)); hit.append(False); kind.append("outside")
    out = dict(pt=np.array(pts, dtype=np.float32), cell=np.array(cells, dtype=np.int64), hit=np.array(hit), kind=kind,
               unplaced=unplaced, n_valid_probes=n_valid_probes, n_valid_cells=len(vk))
    for a in ("pt", "cell", "hit"):
        out[a].setflags(write=False)
    return out


def probes(cat, p):
    """dict: pt float32 [n, dim] | cell int64 [n, dim] (per-axis cell indices; -3 for the point outside) | hit bool [n]
    (the exact valid bit of the cell) | kind [n] (direction and step, 'mean', 'invalid', 'empty', 'corner', 'outside') |
    unplaced [(cell, direction)] | n_valid_probes | n_valid_cells.  The valid cells' probes come first.  Shared: read only."""
    return _probes(cat.name, p)


def describe(cat, p, j):
    pr = probes(cat, p)
    ix = pr["cell"][j]
    at = "outside the grid" if pr["kind"][j] == "outside" else \
        f"cell {tuple(int(v) for v in ix)} ({cat.cell_name(cell_key(ix[None], cat.ext)[0])})"
    return f"{cat.name} {K.PARAMS[p]} probe {j} [{pr['kind'][j]}] at {pr['pt'][j].tolist()} of {at}"


# ---------------------------------------------------------------------------------------------- targets
@functools.lru_cache(maxsize=None)
def _sweep_cloud(name):
    cat = catalogue(name)
    if cat.big is None:
        return cat.cloud
    origin = np.asarray(cat.h["origin"], dtype=np.float32)[0, :cat.dim]
    idx = ((cat.cloud - origin) * np.float32(1.0 / cat.c)).astype(np.int64)
    keep = cell_key(idx, cat.ext) != cat.big
    keep[cat.extent_points()] = True
    assert keep.sum() < 4000 and cat.cells["n"][cat.big] >= (~keep).sum() > 1 << 19
    out = cat.cloud[keep]
    out.setflags(write=False)
    return out


def sweep_cloud(cat):
    """The cloud without the points of a 2^20-point cell (but for cat.extent_points(), so that the grid does not change):
    the target of the per-cell sweeps, about a thousand points.  That cell is not probed on it."""
    return _sweep_cloud(cat.name)


def stretched(cat, cloud, min_cells, max_side=512):
    """(`cloud` plus one point beyond its maximum corner by the same number k of cells on every axis, k, the extents):
    the fewest k that give the grid more than min_cells cells.  The point lies on the maximum side, so the origin and the
    centre of every cell of the catalogue stay what they were, and it sits alone in its cell."""
    top = cloud.max(axis=0).astype(np.float64)
    o0, e0 = R.grid_geometry(cloud, cat.c)
    assert list(e0) == cat.ext
    for k in range(1, max_side):
        more = np.concatenate([cloud, (top + k * cat.c).astype(np.float32)[None]])
        origin, ext = R.grid_geometry(more, cat.c)
        if int(np.prod(ext)) > min_cells:
            assert max(ext) < max_side and np.array_equal(np.asarray(origin), np.asarray(o0)), (cat.name, ext)
            # (k cells up, or k + 1 where the float32 rounding of the far coordinate lands on the next face)
            assert all(e0[a] + k <= e <= e0[a] + k + 1 for a, e in enumerate(ext)), (cat.name, k, ext)
            return more, k, [int(e) for e in ext]
    raise AssertionError((cat.name, min_cells))


# ---------------------------------------------------------------------------------------------- the terms
FLUSH = 2.0 ** -102         # float32's smallest normal number, 2^-126, in units of u: a smaller result may be flushed to zero


class _RE:
    """A float64 value with its running-error scale e (in roundings of relative size 1: |computed - v| <= u e to first
    order for a float32 evaluation with unit roundoff u = eps32 / 2).  Exact operations are charged nothing; a product
    and the score are charged FLUSH on top of their size (a probe in a neighbouring grid's cell, twenty sigma out, has a
    score of 1e-95: zero in float32)."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else e

    def _zero(self):
        return (self.e == 0.0) & (self.v == 0.0)

    def _unit(self):
        return (self.e == 0.0) & ((self.v == 0.0) | (np.abs(self.v) == 1.0))

    def __neg__(self):
        return _RE(-self.v, self.e)

    def __add__(self, o):
        v = self.v + o.v
        return _RE(v, self.e + o.e + np.where(self._zero() | o._zero(), 0.0, np.abs(v)))

    def __sub__(self, o):
        return self + (-o)

    def __mul__(self, o):
        with np.errstate(invalid="ignore", over="ignore"):
            return self._mul(o)

    def _mul(self, o):
        v = self.v * o.v
        return _RE(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + np.where(self._unit() | o._unit(), 0.0, np.abs(v) + FLUSH))

    def score(self, d1, d2):
        """d1 exp(-d2 / 2 m): the scaled argument (a rounded constant and a product: two roundings), the exponential
        (1 ulp = two roundings)."""
        x = -0.5 * d2 * self.v
        with np.errstate(over="ignore"):
            s = d1 * np.exp(x)
        return _RE(s, s * (0.5 * d2 * self.e + 2.0 * np.abs(x) + 2.0) + FLUSH)


def _sym(rows, dim):
    """record rows [n, nsym] -> dim x dim nested list of _RE"""
    C = [[None] * dim for _ in range(dim)]
    for p, (a, b) in enumerate(X.PAIRS[dim]):
        C[a][b] = C[b][a] = _RE(rows[:, p])
    return C


def _dot(xs, ys):
    t = xs[0] * ys[0]
    for x, y in zip(xs[1:], ys[1:]):
        t = t + x * y
    return t


# d2R / da db at the identity (R = Rz Ry Rx; a <= b over roll, pitch, yaw): products of the generators below
_G = [np.array(m, dtype=np.float64) for m in ([[0, 0, 0], [0, 0, -1], [0, 1, 0]], [[0, 0, 1], [0, 0, 0], [-1, 0, 0]],
                                              [[0, -1, 0], [1, 0, 0], [0, 0, 0]])]
_DD = {(a, b): _G[b] @ _G[a] for a in range(3) for b in range(a, 3)}


def terms(dim, pt, mean, icov, mode=0, d1=1.0, d2=1.0):
    """The per-point terms of docs/ALGORITHM.md 2.4 (dim 2) / 2.6 (dim 3) at the identity pose for image points
    pt [n, dim] and records mean [n, dim], icov [n, nsym]; mode 1: the Newton form.  Returns (out [n, nout], A [n, nout]):
    H row-major, g, score as float64, and the running-error scale of each entry."""
    pt = np.asarray(pt, dtype=np.float64)
    mean, icov = np.asarray(mean, dtype=np.float64), np.asarray(icov, dtype=np.float64)
    n, npose = len(pt), NPOSE[dim]
    p = [_RE(pt[:, a]) for a in range(dim)]
    q = [p[a] - _RE(mean[:, a]) for a in range(dim)]
    C = _sym(icov, dim)
    v = [_dot(C[a], q) for a in range(dim)]
    s = _dot(q, v).score(d1, d2)
    w = s * _RE(np.full(n, float(d2)))
    zero, one = _RE(np.zeros(n)), _RE(np.ones(n))
    # the columns of J = [I | dR/dangle p] at the identity: entries 0, +-1, +-coordinates
    J = [[one if a == k else zero for a in range(dim)] for k in range(dim)]
    if dim == 2:
        J.append([-p[1], p[0]])
    else:
        J += [[zero, -p[2], p[1]], [p[2], zero, -p[0]], [-p[1], p[0], zero]]
    Jv = [_dot(J[k], v) for k in range(npose)]
    CJ = [[_dot(C[a], J[k]) for a in range(dim)] for k in range(npose)]
    H = [[None] * npose for _ in range(npose)]
    for k in range(npose):
        for l in range(k, npose):
            h = _dot(J[k], CJ[l])
            if mode == 1:
                h = h - _RE(np.full(n, float(d2))) * Jv[k] * Jv[l]
                if dim == 2 and k == l == 2:                        # v' d2p'/dtheta2, d2p'/dtheta2 = -p
                    h = h - _dot(v, p)
                if dim == 3 and k >= 3:                             # v' (d2R / da db) p
                    D = _DD[(k - 3, l - 3)]
                    for a in range(3):
                        for b in range(3):
                            if D[a, b] != 0.0:
                                h = h + _RE(np.full(n, D[a, b])) * (v[a] * p[b])
            H[k][l] = H[l][k] = w * h
    cols = [H[k][l] for k in range(npose) for l in range(npose)] + [w * Jv[k] for k in range(npose)] + [s]
    return np.stack([t.v for t in cols], axis=1), np.stack([t.e for t in cols], axis=1)


def values(dim, pt, mean, icov, mode=0, d1=1.0, d2=1.0):
    """out of terms() alone, as plain matrix products: what the storage part evaluates some thirty times per probe
    (tolerance() checks it against terms() at every base point)."""
    pt, mean, icov = (np.asarray(a, dtype=np.float64) for a in (pt, mean, icov))
    n, npose = len(pt), NPOSE[dim]
    C = np.zeros((n, dim, dim))
    for k, (a, b) in enumerate(X.PAIRS[dim]):
        C[:, a, b] = C[:, b, a] = icov[:, k]
    q = pt - mean
    v = np.einsum("nab,nb->na", C, q)
    with np.errstate(over="ignore", invalid="ignore"):
        s = d1 * np.exp(-0.5 * d2 * np.einsum("na,na->n", q, v))
        w = s * d2
        J = np.zeros((n, dim, npose))
        for a in range(dim):
            J[:, a, a] = 1.0
        if dim == 2:
            J[:, 0, 2], J[:, 1, 2] = -pt[:, 1], pt[:, 0]
        else:
            for k in range(3):
                J[:, :, 3 + k] = pt @ _G[k].T
        Jv = np.einsum("nak,na->nk", J, v)
        H = np.einsum("nak,nab,nbl->nkl", J, C, J)
        if mode == 1:
            H = H - d2 * Jv[:, :, None] * Jv[:, None, :]
            if dim == 2:
                H[:, 2, 2] -= np.einsum("na,na->n", v, pt)
            else:
                for (a, b), D in _DD.items():
                    t = np.einsum("na,ab,nb->n", v, D, pt)
                    H[:, 3 + a, 3 + b] += t
                    if a != b:
                        H[:, 3 + b, 3 + a] += t
        return np.concatenate([(w[:, None, None] * H).reshape(n, -1), w[:, None] * Jv, s[:, None]], axis=1)


def tolerance(dim, pt, rec, keys, centre, c, mode=0, c_record=X.C_RECORD, c_probe=None):
    """(out [n, nout], tolerance [n, nout], arithmetic part [n, nout], alt) for probes pt [n, dim] of the cells `keys` of
    the records `rec` (exact, or records_float64 with c_record = 2 C_RECORD), `centre` [n, dim] their centres.
    alt = {row: [(out, tolerance, arithmetic part) rows]}: further admissible references of a probe whose cell's mean
    lies on a float32 rounding tie (see the module docstring); a device row has to meet one of them."""
    pt = np.asarray(pt, dtype=np.float64)
    mean, icov = rec["mean"][keys], rec["icov"][keys]
    slack = X.mean_tolerance(mean, centre, c, c_record, stored32=False)
    lo, hi = ((mean + s * slack).astype(np.float32).astype(np.float64) for s in (-1.0, 1.0))
    it = X.matrix_tolerance(icov, rec["kappa"][keys], c_record)
    cp = C_PROBE[dim] if c_probe is None else c_probe

    def at(rows, mu):
        x, t, p = icov[rows], it[rows], pt[rows]
        out, A = terms(dim, p, mu, x, mode)
        f = lambda moved: values(dim, p, mu, moved, mode)
        assert np.all(np.abs(f(x) - out) <= 1e-12 * A + 1e-300), "values() and terms() disagree"
        free = [j for j in range(x.shape[1]) if t[:, j].any()]
        store = np.zeros_like(out)
        plus = {}
        for j in free:
            step = np.zeros_like(x)
            step[:, j] = t[:, j]
            plus[j] = f(x + step) - out
            store += np.maximum(np.abs(plus[j]), np.abs(f(x - step) - out))
        # the interaction of two entries: what moving both changes beyond the separate moves.  Second order, and still
        # what is left where the first order cancels - the Newton H of an isotropic cell one sigma out is
        # w c_yz (1 - m)  at m = 1
        for i, j in enumerate(free):
            for k in free[i + 1:]:
                step = np.zeros_like(x)
                step[:, j], step[:, k] = t[:, j], t[:, k]
                store += np.abs(f(x + step) - out - plus[j] - plus[k])
        tol = store + cp * EPS32 * A
        return out, np.where(np.isnan(tol), np.inf, tol), cp * EPS32 * A     # (a moved record that overflows the score: no bound)

    out, tol, arith = at(np.arange(len(pt)), lo)
    alt = {}
    tied = lo != hi
    for mask in range(1, 1 << dim):                  # the coordinates that take the upper neighbour
        up = np.array([bool(mask >> a & 1) for a in range(dim)])
        rows = np.flatnonzero(np.all(tied | ~up, axis=1))
        if rows.size:
            o, t, ar = at(rows, np.where(up, hi[rows], lo[rows]))
            for j, r in enumerate(rows):
                alt.setdefault(int(r), []).append((o[j], t[j], ar[j]))
    return out, tol, arith, alt


class Reference:
    """hit [n] | out, tol, arith [n, nout] | alt {row: [(out, tol, arith) rows]}: what the rows of a batch call over some
    probes are held to.  Rows of probes that miss are zero with zero tolerance."""

    def __init__(self, hit, out, tol, arith, alt):
        self.hit, self.out, self.tol, self.arith, self.alt = hit, out, tol, arith, alt

    def select(self, sel):
        where = {int(k): j for j, k in enumerate(sel)}
        return Reference(self.hit[sel], self.out[sel], self.tol[sel], self.arith[sel],
                         {where[r]: v for r, v in self.alt.items() if r in where})

    def ratios(self, got):
        """per row (the largest |got - out| / tol, its entry), against the admissible reference that fits the row best"""
        r = _ratio(got, self.out, self.tol)
        for row, others in self.alt.items():
            for o, t, _ in others:
                q = _ratio(got[row], o, t)
                if q.max() < r[row].max():
                    r[row] = q
        return r.max(axis=1), r.argmax(axis=1)

    def worst(self, got):
        """(the largest ratio, (row, entry))"""
        if len(got) == 0:
            return 0.0, (0, 0)
        r, e = self.ratios(got)
        j = int(np.argmax(r))
        return float(r[j]), (j, int(e[j]))

    def arith_bound(self):
        """the arithmetic part, the largest over the admissible references of a row"""
        a = self.arith.copy()
        for row, others in self.alt.items():
            for _, _, ar in others:
                a[row] = np.maximum(a[row], ar)
        return a


def _ratio(got, out, tol):
    """|got - out| / tol per entry; an entry with zero tolerance must be equal, a NaN fails: both give inf"""
    err = np.abs(got - out)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0.0, err / np.where(tol > 0.0, tol, 1.0), np.where(err == 0.0, 0.0, np.inf))
    return np.where(np.isnan(r), np.inf, r)


@functools.lru_cache(maxsize=None)
def _exact_reference(name, p, mode):
    ref = _reference(catalogue(name), p, mode, None, X.C_RECORD)
    for a in (ref.out, ref.tol, ref.arith):
        a.setflags(write=False)
    return ref


def reference(cat, p, mode=0, rec=None, c_record=X.C_RECORD):
    """The Reference of all probes of (cat, p) against the exact records (computed once and shared: read only) or
    against `rec`."""
    return _exact_reference(cat.name, p, mode) if rec is None else _reference(cat, p, mode, rec, c_record)


def _reference(cat, p, mode, rec, c_record):
    pr = probes(cat, p)
    rec = K.golden(cat, p) if rec is None else rec
    nv = pr["n_valid_probes"]
    keys = cell_key(pr["cell"][:nv], cat.ext)
    assert rec["valid"][keys].all()
    ctr = X.all_centres(cat.h)[keys]
    out = np.zeros((len(pr["pt"]), nout(cat.dim)))
    tol, arith = np.zeros_like(out), np.zeros_like(out)
    out[:nv], tol[:nv], arith[:nv], alt = tolerance(cat.dim, pr["pt"][:nv].astype(np.float64), rec, keys, ctr, cat.c, mode, c_record)
    return Reference(pr["hit"], out, tol, arith, alt)


def row_vector(dim, H, g, score):
    """a result's H, g, score in the layout of terms()"""
    return np.concatenate([np.asarray(H, dtype=np.float64).reshape(-1), np.asarray(g, dtype=np.float64), [float(score)]])


# ---------------------------------------------------------------------------------------------- the oracle's float32 mirror
def mirror_terms(dim, pt32, mean32, icov32, mode):
    """oracle.ndt2d.evaluate / oracle.ndt3d.evaluate3 with mirror32=True for one float32 point on a one-cell grid that
    holds one float32 record (the grid's origin a quarter of a cell below the point), at the identity pose."""
    from oracle import ndt2d as o2, ndt3d as o3
    c = 1.0
    o = (pt32.astype(np.float64) - 0.25 * c).astype(np.float32)
    one = np.ones(1, dtype=np.int64)
    coords = [pt32[a:a + 1] for a in range(dim)]
    if dim == 2:
        grid = o2.Grid2D(o[0], o[1], np.float32(1.0 / c), 1, 1, one, mean32[None].astype(np.float64),
                         icov32[None].astype(np.float64), np.ones(1, bool), 1)
        H, g, sc, nh = o2.evaluate(grid, *coords, (0.0, 0.0, 0.0), o2.NdtParams(cell_size=c, hessian_mode=mode), mirror32=True)
    else:
        grid = o3.Grid3D(o, np.float32(1.0 / c), (1, 1, 1), one, mean32[None].astype(np.float64),
                         icov32[None].astype(np.float64), np.ones(1, bool), 1)
        H, g, sc, nh = o3.evaluate3(grid, *coords, (0.0,) * 6, o3.Ndt3Params(cell_size=c, hessian_mode=mode), mirror32=True)
    assert nh == 1
    return row_vector(dim, H, g, sc)
