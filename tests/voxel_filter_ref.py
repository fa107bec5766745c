"""The exact reference of the voxel-grid scan filter (docs/ALGORITHM.md section 2.24), point by point with Python floats,
integers and fractions.Fraction - independent in form of gtsam_ndt_amd/voxel.py and of the kernels.  Keys and U come
from the contract's float64 expressions (a Python float is an IEEE double, each operator rounds once, round() rounds
half to even); the centroid is then the EXACT rational X = centre + sum U leaf / (n 2^22), which the contract's output
(one rounded division, one fma, one rounding to float32) approaches within bound()."""
import math
from fractions import Fraction

import numpy as np

FIX = 1 << 22
LIMIT = 1 << 30
EPS64 = 2.0 ** -53


def reference(coords, leaf, min_points=1):
    """coords [n, dim] float32 -> dict: keys [m] tuples (ix, iy[, iz]) in the contract's order, counts [m], X [m][dim]
    Fractions, centre [m][dim] floats, and info (n_invalid, n_voxels, n_out)."""
    coords = np.asarray(coords, dtype=np.float32)
    dim = coords.shape[1]
    leaf = float(leaf)
    scale = float(FIX) / leaf
    cells = {}
    n_invalid = 0
    for row in coords:
        key, us = [], []
        for v in row:
            x = float(v)
            if not math.isfinite(x):
                break
            q = x / leaf
            if not math.isfinite(q):
                break
            i = math.floor(q)
            if abs(i) >= LIMIT:
                break
            centre = (i + 0.5) * leaf
            key.append(i)
            us.append(round((x - centre) * scale))
        if len(key) < dim:
            n_invalid += 1
            continue
        acc = cells.setdefault(tuple(key), [0] + [0] * dim)
        acc[0] += 1
        for d in range(dim):
            acc[1 + d] += us[d]
    order = sorted(cells, key=lambda k: k[::-1])
    keys, counts, X, centres = [], [], [], []
    for k in order:
        n = cells[k][0]
        if n < min_points:
            continue
        c = [(i + 0.5) * leaf for i in k]
        keys.append(k)
        counts.append(n)
        centres.append(c)
        X.append([Fraction(c[d]) + Fraction(cells[k][1 + d]) * Fraction(leaf) / (n * FIX) for d in range(dim)])
    return dict(keys=keys, counts=counts, X=X, centre=centres, info=(n_invalid, len(cells), len(keys)))


def ulp32(x):
    """The spacing of float32 at |x| (x a Fraction or float), at least that of the smallest normal binade."""
    a = abs(float(x))
    return 2.0 ** (max(math.frexp(a)[1] - 1, -126) - 23) if a > 0.0 else 2.0 ** -149


def bound(X, centre, leaf):
    """1/2 ulp32(X) + 2 eps64 (|centre| + leaf): the float32 rounding of the output; and ahead of it the rounded division
    leaf / (n 2^22), whose relative error eps64 scales a term of at most leaf / 2, and the fma's rounding of a double
    below |centre| + leaf - together less than 2 eps64 (|centre| + leaf).  Derived, not measured."""
    return 0.5 * ulp32(X) + 2.0 * EPS64 * (abs(centre) + leaf)


def check(points, counts, info, ref, leaf):
    """Asserts that an implementation's (points [m, dim] float32, counts [m], info triple) meets the reference: counts,
    order and info exactly, every coordinate within bound() of X.  Returns the largest error / bound."""
    points = np.asarray(points)
    assert tuple(int(v) for v in info) == ref["info"], (tuple(info), ref["info"])
    assert points.dtype == np.float32 and points.shape == (len(ref["keys"]), points.shape[1])
    assert [int(c) for c in counts] == ref["counts"]
    worst = 0.0
    for v in range(points.shape[0]):
        for d in range(points.shape[1]):
            X, c = ref["X"][v][d], ref["centre"][v][d]
            # the order is checked through the coordinates: a point lies in (the closure of) its voxel, up to the bound
            err = abs(Fraction(float(points[v, d])) - X)
            b = bound(X, c, leaf)
            assert err <= b, (v, d, float(err), b, ref["keys"][v])
            worst = max(worst, float(err) / b)
    return worst
