"""The definition of submap coarsening (docs/ALGORITHM.md section 2.17, tests/map_coarsen_ref.py) against a direct binning
of the same points at the coarse cell size: no GPU.  Fine blobs are built in numpy by the documented formula
U = rint((p - centre) 2^22 / c)."""
import numpy as np
import pytest

import map_coarsen_ref as R


def dyadic_cloud(seed, n, dim, span=64.0, bits=11):
    """Coordinates that are odd multiples of 2^-bits within +-span: every float32 step of the binning is exact for the
    cell sizes used here, and no point lies on a cell boundary."""
    rng = np.random.default_rng(seed)
    m = rng.integers(-int(span * 2 ** (bits - 1)), int(span * 2 ** (bits - 1)), size=(n, dim))
    centres = rng.uniform(-span * 0.8, span * 0.8, size=(12, dim))           # clustered: cells of many points
    pick = rng.integers(0, 12, size=n)
    m = np.where(rng.random((n, 1)) < 0.7, np.rint((centres[pick] + rng.normal(0, 1.5, (n, dim))) * 2 ** (bits - 1)), m)
    m = np.clip(m, -int(span * 2 ** (bits - 1)), int(span * 2 ** (bits - 1)) - 1).astype(np.int64)
    return ((2 * m + 1) * 2.0 ** -bits).astype(np.float32)


def assert_binning_exact(pts, c, f):
    """What the comparison rests on, asserted: the float32 binning of both cell sizes equals the exact one, and every
    point's coarse cell is the parent of its fine cell."""
    assert np.array_equal(pts.astype(np.float64).astype(np.float32), pts)
    out = []
    for cell in (c, f * c):
        origin, ext = R.grid_geometry(pts, cell)
        _, idx, fidx = R.blob_from_points(pts, cell)
        exact = (pts.astype(np.float64) - origin.astype(np.float64)) / cell
        assert np.array_equal(idx, np.floor(exact).astype(np.int64))
        assert np.all(exact != np.floor(exact))
        assert np.all(idx >= 1) and np.all(idx <= np.array(ext) - 2)
        out.append((origin, ext, idx))
    (of, ef, idf), (oc, ec, idc) = out
    for a in range(pts.shape[1]):
        k0, K0, off, extent = R.coarsen_axis(of[a], c, ef[a], f)
        assert extent == ec[a] and np.float32(K0 * c) == oc[a]
        assert np.array_equal((off + idf[:, a]) // f, idc[:, a])


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("c", [0.5, 1.0])
@pytest.mark.parametrize("f", [2, 4])
def test_coarsened_equals_direct_binning_within_the_bounds(dim, c, f):
    pts = dyadic_cloud(11 * dim + f, 2500, dim, span=64.0 if dim == 2 else 16.0)     # (3D: a grid of a few MB)
    assert np.abs(pts).max() < 64.0
    assert_binning_exact(pts, c, f)
    fine, idx, _ = R.blob_from_points(pts, c)
    coarse = R.map_coarsen_ref(fine, f)
    direct, _, _ = R.blob_from_points(pts, f * c)
    R.check_against_direct(coarse, direct, f)
    hf, cf = R.parse(fine)
    hc, cc = R.parse(coarse)
    assert int(cc["n"].sum()) == int(cf["n"].sum()) == len(pts)
    assert hc["n_points"] == hf["n_points"]


@pytest.mark.parametrize("dim,c,f", [(2, 0.5, 4), (2, 1.0, 4), (3, 1.0, 4), (3, 0.5, 2)])
def test_bounds_hold_where_the_roundings_bite(dim, c, f):
    """Coordinates on a 2^-23 lattice within +-2 m: the fixed-point coordinates are no integers before rounding (fine at
    c = 1, direct always), so the differences are not zero.  (The float32 subtraction p - o may round here; the test
    asserts that no point's cell changes by it.)"""
    rng = np.random.default_rng(5 + dim + f)
    m = rng.integers(-2 ** 23, 2 ** 23, size=(4000, dim))
    pts = ((2 * m + 1) * 2.0 ** -23).astype(np.float32)
    for cell in (c, f * c):
        origin, ext = R.grid_geometry(pts, cell)
        _, idx, _ = R.blob_from_points(pts, cell)
        assert np.array_equal(idx, np.floor((pts.astype(np.float64) - origin.astype(np.float64)) / cell).astype(np.int64))
    fine, _, _ = R.blob_from_points(pts, c)
    direct, _, _ = R.blob_from_points(pts, f * c)
    worst = R.check_against_direct(R.map_coarsen_ref(fine, f), direct, f)
    assert worst[0] > 0 and worst[1] > 0          # the roundings did bite


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("f", [2, 4])
def test_counts_are_conserved_cell_by_cell(dim, f):
    pts = dyadic_cloud(3, 3000, dim, span=20.0)
    fine, idx, _ = R.blob_from_points(pts, 0.5)
    hf, cf = R.parse(fine)
    hc, cc = R.parse(R.map_coarsen_ref(fine, f))
    ext = [hf["width"], hf["height"], hf["depth"]][:dim]
    cext = [hc["width"], hc["height"], hc["depth"]][:dim]
    want = np.zeros(cc.size, dtype=np.int64)
    par = []
    for a in range(dim):
        _, _, off, extent = R.coarsen_axis(hf["origin"][0][a], 0.5, ext[a], f)
        assert extent == cext[a]
        par.append((off + idx[:, a]) // f)
    k = par[0] + cext[0] * (par[1] + (cext[1] * par[2] if dim == 3 else 0))
    np.add.at(want, k, 1)
    assert np.array_equal(want, cc["n"].astype(np.int64))
    if dim == 2:                                   # the empty-ring contract of 2D grids
        n2 = cc["n"].reshape(cext[1], cext[0])
        assert not n2[0].any() and not n2[-1].any() and not n2[:, 0].any() and not n2[:, -1].any()


@pytest.mark.parametrize("k0,w,f", [(-7, 13, 2), (-7, 13, 4), (-5, 3, 4), (0, 10, 2), (3, 9, 4), (-1, 6, 4), (-4, 8, 4)])
def test_lattice_of_one_axis(k0, w, f):
    c = 0.5
    got_k0, K0, off, extent = R.coarsen_axis(np.float32(k0 * c), c, w, f)
    assert got_k0 == k0 and K0 % f == 0 and f - 1 <= off <= 2 * f - 2
    # what ndt*_set_target derives at cell f c from a cloud whose fine lattice this is: first interior fine cell k0 + 1
    assert K0 == f * (int(np.floor((k0 + 1) / f)) - 1)
    assert all((off + ix) // f >= 1 for ix in range(1, w))                        # coarse cell 0: ring or outside only
    assert (off + w - 2) // f == extent - 2                                       # last interior fine cell
    assert (off + w - 1) // f <= extent - 1                                       # the ring stays inside


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("f", [2, 4])
def test_degenerate_cell_passes_the_plausibility_check(dim, f):
    """Five identical points near a corner of their coarse cell: n SS = S^2 exactly for a point set, and the two roundings
    must not leave it below (ndt*_load_map refuses such a cell as forged)."""
    c = 0.5
    pairs = [(a, b) for a in range(dim) for b in range(a, dim)]
    needed = 0
    for seed in range(16):
        rng = np.random.default_rng(seed)
        corner = (rng.integers(-1, 1, size=dim) * f * c).astype(np.float64)   # |p| < 2: 2^-23 is a float32 step
        p = corner + f * c - (2 * rng.integers(0, 300, size=dim) + 1) * 2.0 ** -23        # just inside the upper corner
        frame = np.array([corner - 3 * f * c, corner + 4 * f * c])
        pts = np.vstack([np.repeat(p[None, :], 5, axis=0), frame]).astype(np.float32)
        fine, _, _ = R.blob_from_points(pts, c)
        for clamp in (True, False):
            h, cells = R.parse(R.map_coarsen_ref(fine, f, clamp=clamp))
            k = int(np.flatnonzero(cells["n"] == 5)[0])
            s = [int(v) for v in cells["s"][k]]
            ss = [int(v) for v in cells["ss"][k]]
            dg = [ss[i] for i, (a, b) in enumerate(pairs) if a == b]
            off = [ss[i] for i, (a, b) in enumerate(pairs) if a != b]
            if clamp:
                assert R.cell_sums_plausible(5, s, dg, off)
            else:
                needed += not R.cell_sums_plausible(5, s, dg, off)
    assert needed > 0                              # without the clamp some of these cells are refused


def test_reference_refuses_what_the_library_refuses():
    pts = dyadic_cloud(1, 500, 2, span=10.0)
    fine, _, _ = R.blob_from_points(pts, 0.5)
    for f in (1, 3, 8):
        with pytest.raises(R.CoarsenError):
            R.map_coarsen_ref(fine, f)
    with pytest.raises(R.CoarsenError):
        R.map_coarsen_ref(fine[:100], 2)
    bad = fine.copy(); bad[0] ^= 1
    with pytest.raises(R.CoarsenError):
        R.map_coarsen_ref(bad, 2)
    h, cells = R.parse(fine)
    four = dict(h, ngrid=4, n_cells=4 * h["n_cells"])
    with pytest.raises(R.CoarsenError):
        R.map_coarsen_ref(R.pack(four, np.concatenate([cells] * 4)), 2)
    # one parent fed by four children of 300 000 points each
    big = cells.copy()
    big[:] = 0
    W = h["width"]
    _, _, offx, _ = R.coarsen_axis(h["origin"][0][0], 0.5, W, 2)
    _, _, offy, _ = R.coarsen_axis(h["origin"][0][1], 0.5, h["height"], 2)
    ix, iy = 2 + (offx % 2), 2 + (offy % 2)                  # first child of a parent
    for dy in (0, 1):
        for dx in (0, 1):
            big["n"][(iy + dy) * W + ix + dx] = 300000
    with pytest.raises(R.CoarsenError, match="2\\^20"):
        R.map_coarsen_ref(R.pack(h, big), 2)
