"""The per-cell records (docs/ALGORITHM.md sections 2.2, 2.3, 2.6) from a save_map blob, twice:

exact_cells(blob).records(min_points, eig_ratio)
    The exact answer.  mu = centre + Su / (n S) and Sigma = (n Suu - Su Su^T) / (n (n - 1) S^2) as Python integers and
    fractions.Fraction (S = 2^22 / c, centre = the float64 value fma(i + 0.5, c, o) taken exactly), validity on the
    integers, the symmetric eigenproblem and the spectral functions  lambda -> 1 / max(lambda, eig_ratio lambda_max)
    (Sigma^-1)  and  lambda -> max(lambda, eig_ratio lambda_max)  (Sigma)  with mpmath at 60 digits.  It knows nothing
    of oracle/ nor of the order in which the kernels operate; it needs mpmath, so its results are committed as
    tests/golden/cell_records.npz for the GPU tests.

records_float64(blob, min_points, eig_ratio)
    The documented device formula restated in float64 numpy: the numerator n Suu - Su Su as an exact integer, rounded
    once; 2D r = 1 / (n S), mu = Su r + centre, M2 = num r^2 n, Sigma = M2 / (n - 1), closed-form eigenvalues and the
    better conditioned eigenvector formula; 3D Sigma = num / (n S^2 (n - 1)) and six cyclic Jacobi sweeps over
    (0,1), (0,2), (1,2).  `mutant` switches one deliberate mistake on (tests/test_cell_record_ref.py).

Both return a dict of arrays over the blob's cells (all `ngrid` grids, in the blob's order):
    valid bool [k] | mean float64 [k, dim] | icov float64 [k, nsym] | cov float64 [k, nsym] | kappa float64 [k]
with nsym = 3 (xx xy yy) or 6 (xx xy xz yy yz zz), zero rows for invalid cells, and
kappa = lambda_max / min_k max(lambda_k, eig_ratio lambda_max).

THE TOLERANCE of a stored (float32) record entry x against its exact value X, for a cell whose matrix (Sigma^-1 or Sigma,
as clamped) has Frobenius norm N:

    |x - X| <= ulp32(X) / 2 + C_RECORD eps64 kappa N                      (means: |centre| + cell_size for kappa N)

The first term is the float32 store, the second float64 rounding through an eigen-decomposition of condition kappa.
C_RECORD is measured, by the rule of tests/step_replay.py: test_cell_record_ref.test_float64_error_is_an_eighth_of_the_
tolerance takes the worst error of records_float64 and of oracle/ (finalise_cell, finalise_cells3 fed the exact
moments) against the exact records over both catalogues of tests/cell_record_cases.py and every parameter set, in units
of eps64 kappa N:

    MEASURED_UNITS = 3.48    (records_float64 and oracle alike, 3D Sigma^-1 of cell 913 of catalogue far3_5 with min_points 3,
                              eig_ratio 1: kappa 1, every eigenvalue clamped to the largest.  Per source and dimension:
                              records_float64 2D 1.90, 3D 3.48; oracle, Sigma^-1 only, 2D 0.84, 3D 3.48; the means come
                              out correctly rounded, 0 units.  At kappa = 1e6 the worst is 0.31 unit: the bound is looser
                              there, not tighter.)
    C_RECORD = 8 * MEASURED_UNITS, rounded up = 28

In the metric of the older parity tests (max |delta| / ||Sigma^-1||_F < 1e-5) this bound is at most
6e-8 + 28 eps64 kappa = 6e-8 + 6.2e-15 kappa: 150 times tighter than 1e-5 for every kappa up to 1e6, and it holds each
entry to its own float32 ulp - where 1e-5 of the norm allowed, at kappa = 1e6, an error of ten times the small entries
themselves."""
from fractions import Fraction

import numpy as np

import map_coarsen_ref as R

EPS64 = 2.0 ** -52
MEASURED_UNITS = 3.48
C_RECORD = 28.0
PAIRS = {2: ((0, 0), (0, 1), (1, 1)), 3: ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))}


# ---------------------------------------------------------------------------------------------- geometry of a blob
def geometry(h):
    """(dim, extents, cell size, origins [ngrid, dim] as float32)."""
    dim = h["dims"]
    ext = [h["width"], h["height"], h["depth"]][:dim]
    return dim, ext, float(h["cell_size"]), np.asarray(h["origin"], dtype=np.float32)[:h["ngrid"], :dim]


def cell_index(k, ext):
    """cell number within one grid -> per-axis indices [len(k), dim] (x fastest)."""
    k = np.asarray(k, dtype=np.int64)
    out = [k % ext[0], (k // ext[0]) % ext[1]]
    if len(ext) == 3:
        out.append(k // (ext[0] * ext[1]))
    return np.stack(out, axis=1)


def centres(h, k):
    """float64 centres fma(i + 0.5, c, o) [len(k), dim] of the blob's cells k (numbered across all grids), exactly:
    the sum is formed as a fraction and rounded once."""
    dim, ext, c, origin = geometry(h)
    ncell = int(np.prod(ext))
    k = np.asarray(k, dtype=np.int64)
    idx = cell_index(k % ncell, ext)
    q = k // ncell
    fc = Fraction(c)
    out = np.zeros((len(k), dim))
    for j in range(len(k)):
        for a in range(dim):
            out[j, a] = float(Fraction(2 * int(idx[j, a]) + 1, 2) * fc + Fraction(float(origin[q[j], a])))
    return out


def _empty(ncell, dim):
    ns = len(PAIRS[dim])
    return dict(valid=np.zeros(ncell, bool), mean=np.zeros((ncell, dim)), icov=np.zeros((ncell, ns)),
                cov=np.zeros((ncell, ns)), kappa=np.zeros(ncell))


# ---------------------------------------------------------------------------------------------- the exact reference
class exact_cells:
    """Everything about a blob's cells that does not depend on min_points / eig_ratio, computed once: exact mean,
    exact Sigma, its eigen-decomposition at 60 digits."""
    DPS = 60

    def __init__(self, blob):
        import mpmath
        self.mp = mpmath.mp.clone()
        self.mp.dps = self.DPS
        mp = self.mp
        self.h, cells = R.parse(blob)
        self.dim, self.ext, c, _ = geometry(self.h)
        dim = self.dim
        S = Fraction(1 << 22) / Fraction(c)
        self.n = cells["n"].astype(np.int64)
        self.occupied = np.flatnonzero((self.n >= 2) & (self.n <= R.MAX_CELL_COUNT))
        ctr = centres(self.h, self.occupied)
        self.cells = {}
        for j, k in enumerate(self.occupied):
            n = int(self.n[k])
            s = [int(v) for v in cells["s"][k]]
            ss = [int(v) for v in cells["ss"][k]]
            num = [n * ss[p] - s[a] * s[b] for p, (a, b) in enumerate(PAIRS[dim])]
            trace = sum(num[p] for p, (a, b) in enumerate(PAIRS[dim]) if a == b)
            mean = [float(Fraction(float(ctr[j, a])) + Fraction(s[a]) / (n * S)) for a in range(dim)]
            if trace <= 0:                                   # all points coincide: decided on the integers
                self.cells[int(k)] = (mean, None, None)
                continue
            den = n * (n - 1) * S * S
            A = mp.zeros(dim)
            for p, (a, b) in enumerate(PAIRS[dim]):
                f = Fraction(num[p]) / den
                A[a, b] = A[b, a] = mp.mpf(f.numerator) / mp.mpf(f.denominator)
            E, Q = mp.eigsy(A)
            self.cells[int(k)] = (mean, [E[i] for i in range(dim)], Q)

    def records(self, min_points, eig_ratio):
        mp, dim = self.mp, self.dim
        out = _empty(self.n.size, dim)
        er = mp.mpf(float(eig_ratio))
        for k, (mean, lam, Q) in self.cells.items():
            if self.n[k] < max(int(min_points), 2) or lam is None:
                continue
            lmax = max(lam)
            lim = er * lmax
            lc = [max(l, lim) for l in lam]
            out["valid"][k] = True
            out["mean"][k] = mean
            out["kappa"][k] = float(lmax / min(lc))
            for p, (a, b) in enumerate(PAIRS[dim]):
                out["icov"][k, p] = float(mp.fsum(Q[a, i] * Q[b, i] / lc[i] for i in range(dim)))
                out["cov"][k, p] = float(mp.fsum(Q[a, i] * Q[b, i] * lc[i] for i in range(dim)))
        return out


def exact_records(blob, min_points, eig_ratio):
    return exact_cells(blob).records(min_points, eig_ratio)


# ---------------------------------------------------------------------------------------------- the float64 restatement
MUTANTS = ("divide_by_n", "clamp_at_second", "clamp_at_trace", "three_sweeps", "float32_reciprocal", "half_df_gt",
           "float64_numerator")


def numerators(cells, occ, dim, through_float64=False):
    """n Suu - Su Su [len(occ), nsym] as float64: the exact integer rounded once (through_float64: the mutant that forms
    the two products in float64)."""
    out = np.zeros((len(occ), len(PAIRS[dim])))
    if through_float64:
        n = cells["n"][occ].astype(np.float64)
        s = cells["s"][occ].astype(np.float64)
        ss = cells["ss"][occ].astype(np.float64)
        for p, (a, b) in enumerate(PAIRS[dim]):
            out[:, p] = n * ss[:, p] - s[:, a] * s[:, b]
        return out
    n = cells["n"][occ].astype(object)
    s = cells["s"][occ].astype(object)
    ss = cells["ss"][occ].astype(object)
    for p, (a, b) in enumerate(PAIRS[dim]):
        out[:, p] = (n * ss[:, p] - s[:, a] * s[:, b]).astype(np.float64)
    return out


def _centres_float64(h, occ):
    """fma(i + 0.5, c, o) for many cells: (i + 0.5) c is formed in float64 and added - exact whenever the product is
    (every lattice of the catalogue), else within one rounding of it, which the mean's tolerance covers."""
    dim, ext, c, origin = geometry(h)
    ncell = int(np.prod(ext))
    idx = cell_index(occ % ncell, ext)
    return (idx + 0.5) * c + origin.astype(np.float64)[occ // ncell]


def jacobi6(A, sweeps=6):
    """Cyclic Jacobi over (0,1), (0,2), (1,2) on symmetric 3x3 matrices A [k, 3, 3] -> (diagonal [k, 3], V [k, 3, 3]
    eigenvector columns), the rotation of docs/ALGORITHM.md 2.6: t = sign(tau) / (|tau| + sqrt(1 + tau^2))."""
    A = A.copy()
    k = A.shape[0]
    V = np.tile(np.eye(3), (k, 1, 1))
    for _ in range(sweeps):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            r = 3 - p - q
            apq = A[:, p, q].copy()
            on = np.abs(apq) > 1e-300
            with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
                tau = (A[:, q, q] - A[:, p, p]) / (2.0 * apq)
                t = np.where(tau >= 0.0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
            t = np.where(on, t, 0.0)
            c = 1.0 / np.sqrt(1.0 + t * t)
            s = t * c
            A[:, p, p] -= t * apq
            A[:, q, q] += t * apq
            A[:, p, q] = A[:, q, p] = np.where(on, 0.0, apq)
            rp, rq = A[:, r, p].copy(), A[:, r, q].copy()
            A[:, r, p] = A[:, p, r] = c * rp - s * rq
            A[:, r, q] = A[:, q, r] = s * rp + c * rq
            vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
            V[:, :, p] = c[:, None] * vp - s[:, None] * vq
            V[:, :, q] = s[:, None] * vp + c[:, None] * vq
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1), V


def _rcp(x, mutant):
    if mutant == "float32_reciprocal":
        return (np.float32(1.0) / x.astype(np.float32)).astype(np.float64)
    return 1.0 / x


def records_float64(blob, min_points, eig_ratio, mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    h, cells = R.parse(blob)
    dim, ext, c, _ = geometry(h)
    out = _empty(cells.size, dim)
    n_all = cells["n"].astype(np.int64)
    occ = np.flatnonzero((n_all >= max(int(min_points), 2)) & (n_all <= R.MAX_CELL_COUNT))
    if occ.size == 0:
        return out
    S = 4194304.0 / c
    er = float(eig_ratio)
    dn = n_all[occ].astype(np.float64)
    s = cells["s"][occ].astype(np.float64)
    num = numerators(cells, occ, dim, mutant == "float64_numerator")
    ctr = _centres_float64(h, occ)
    div = dn if mutant == "divide_by_n" else dn - 1.0
    if dim == 2:
        r = 1.0 / (dn * S)
        mean = s * r[:, None] + ctr
        v = num * (r * r * dn)[:, None] / div[:, None]
        vxx, vxy, vyy = v[:, 0], v[:, 1], v[:, 2]
        half_tr, half_df = 0.5 * (vxx + vyy), 0.5 * (vxx - vyy)
        disc = np.sqrt(half_df * half_df + vxy * vxy)
        l1, l2 = half_tr + disc, half_tr - disc
        ok = l1 > 0.0
        lim = er * (l2 if mutant == "clamp_at_second" else 2.0 * half_tr if mutant == "clamp_at_trace" else l1)
        l2c = np.maximum(l2, lim)
        first = half_df > 0.0 if mutant == "half_df_gt" else half_df >= 0.0
        ex = np.where(first, half_df + disc, vxy)
        ey = np.where(first, vxy, disc - half_df)
        nrm = np.sqrt(ex * ex + ey * ey)
        iso = ~(nrm > 0.0)
        safe = np.where(iso, 1.0, nrm)
        ex, ey = np.where(iso, 1.0, ex / safe), np.where(iso, 0.0, ey / safe)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            i1, i2 = _rcp(l1, mutant), _rcp(l2c, mutant)
            d = i1 - i2
            icov = np.stack([d * ex * ex + i2, d * ex * ey, d * ey * ey + i2], axis=1)
            d = l1 - l2c
            cov = np.stack([d * ex * ex + l2c, d * ex * ey, d * ey * ey + l2c], axis=1)
            kappa = l1 / l2c
    else:
        mean = (s / dn[:, None]) * (1.0 / S) + ctr
        a = num * (1.0 / (dn * S * S * div))[:, None]
        A = np.zeros((occ.size, 3, 3))
        for p, (i, j) in enumerate(PAIRS[3]):
            A[:, i, j] = A[:, j, i] = a[:, p]
        lam, V = jacobi6(A, 3 if mutant == "three_sweeps" else 6)
        lmax = lam.max(axis=1)
        ok = lmax > 0.0
        base = np.sort(lam, axis=1)[:, 1] if mutant == "clamp_at_second" else lam.sum(axis=1) if mutant == "clamp_at_trace" else lmax
        lc = np.maximum(lam, (er * base)[:, None])
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            inv = _rcp(lc, mutant)
            icov = np.stack([(inv * V[:, i, :] * V[:, j, :]).sum(axis=1) for i, j in PAIRS[3]], axis=1)
            cov = np.stack([(lc * V[:, i, :] * V[:, j, :]).sum(axis=1) for i, j in PAIRS[3]], axis=1)
            kappa = lmax / lc.min(axis=1)
    k = occ[ok]
    out["valid"][k] = True
    out["mean"][k] = mean[ok]
    out["icov"][k] = icov[ok]
    out["cov"][k] = cov[ok]
    out["kappa"][k] = kappa[ok]
    return out


# ---------------------------------------------------------------------------------------------- the tolerance
def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def sym_norm(m):
    """Frobenius norm of the symmetric matrices stored as [k, nsym] rows."""
    m = np.asarray(m, dtype=np.float64)
    if m.shape[1] == 3:
        w = np.array([1.0, 2.0, 1.0])
    else:
        w = np.array([1.0, 2.0, 2.0, 1.0, 2.0, 1.0])
    return np.sqrt((m * m * w).sum(axis=1))


def matrix_tolerance(exact, kappa, c=C_RECORD, stored32=True):
    """Per-entry bound [k, nsym] for Sigma^-1 or Sigma rows `exact` of cells with condition `kappa`."""
    exact = np.asarray(exact, dtype=np.float64)
    tol = (c * EPS64 * np.asarray(kappa) * sym_norm(exact))[:, None] * np.ones_like(exact)
    return tol + 0.5 * ulp32(exact) if stored32 else tol


def mean_tolerance(exact, centre, cell_size, c=C_RECORD, stored32=True):
    exact = np.asarray(exact, dtype=np.float64)
    tol = c * EPS64 * (np.abs(centre) + cell_size)
    return tol + 0.5 * ulp32(exact) if stored32 else tol


def worst_units(got, exact, centre, cell_size, stored32=False, cells=None):
    """The largest error of `got` against `exact` (dicts as above) in units of eps64 kappa N (matrices) and of
    eps64 (|centre| + c) (means), after taking the float32 store's half ulp off when stored32: what is compared with
    C_RECORD.  Returns {field: (units, cell)} over the exact records' valid cells (or over `cells`)."""
    k = np.flatnonzero(exact["valid"]) if cells is None else np.asarray(cells)
    res = {}
    for f in ("mean", "icov", "cov"):
        if f not in got or k.size == 0:
            continue
        err = np.abs(np.asarray(got[f], dtype=np.float64)[k] - exact[f][k])
        if stored32:
            err = np.maximum(err - 0.5 * ulp32(exact[f][k]), 0.0)
        if f == "mean":
            unit = EPS64 * (np.abs(centre[k]) + cell_size)
        else:
            unit = (EPS64 * exact["kappa"][k] * sym_norm(exact[f][k]))[:, None]
        u = (err / unit).max(axis=1)
        j = int(np.argmax(u))
        res[f] = (float(u[j]), int(k[j]))
    return res


def all_centres(h):
    """float64 centres of every cell of the blob [n_cells, dim] (the float64 sum; see _centres_float64)."""
    return _centres_float64(h, np.arange(h["n_cells"], dtype=np.int64))


# ---------------------------------------------------------------------------------------------- a device grid against records
def check_records(got, ref, h, c=C_RECORD, what="", name=lambda k: f"cell {k}"):
    """Assert the float32 arrays `got` ({'mean', 'icov', 'cov'}: any subset, dense over the cells of grid 0) within the
    tolerance of the records `ref` (exact, or records_float64 with c = 2 C_RECORD) on every valid cell of grid 0, and
    zero elsewhere.  Returns {field: (worst error in units of eps64 kappa N beyond the float32 store, cell)}."""
    dim, ext, cell, _ = geometry(h)
    ncell = int(np.prod(ext))
    valid = ref["valid"][:ncell]
    k = np.flatnonzero(valid)
    ctr = all_centres(h)[:ncell]
    for f, arr in got.items():
        arr = np.asarray(arr)
        assert arr.dtype == np.float32 and arr.shape == ref[f][:ncell].shape, (what, f)
        assert not arr[~valid].any() or f == "mean", (what, f, "an invalid cell holds a record")
        want = ref[f][:ncell][k]
        tol = mean_tolerance(want, ctr[k], cell, c) if f == "mean" else matrix_tolerance(want, ref["kappa"][:ncell][k], c)
        r = np.abs(arr[k].astype(np.float64) - want) / tol
        if r.size and not r.max() <= 1.0:                          # (written so that a NaN fails)
            j, col = np.unravel_index(np.argmax(np.where(np.isnan(r), np.inf, r)), r.shape)
            raise AssertionError(f"{what}: {f}[{col}] of {name(int(k[j]))} is {arr[k[j], col]!r}, reference {want[j, col]!r}: "
                                 f"{r[j, col]:.3g} times the tolerance (kappa {ref['kappa'][k[j]]:.3g})")
    sub = {f: np.asarray(v) for f, v in got.items()}
    dense = {f: ref[f][:ncell] for f in ("valid", "mean", "icov", "cov", "kappa")}
    return worst_units(sub, dense, ctr, cell, stored32=True)
