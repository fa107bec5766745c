"""The voxel-grid scan filter without a device (docs/ALGORITHM.md section 2.24): the numpy restatement
gtsam_ndt_amd/voxel.py against the exact reference tests/voxel_filter_ref.py - keys, counts and order exactly, every
coordinate within 1/2 ulp32(X) + 2 eps64 (|centre| + leaf) of the exact rational centroid X - over a catalogue of the
cases where a filter goes wrong, its invariance under permutation, and its emulated fma against exact arithmetic."""
from fractions import Fraction

import numpy as np
import pytest

import voxel_filter_ref as R
from gtsam_ndt_amd import voxel

LEAVES = (0.25, 0.3)


def _against_reference(pts, leaf, min_points=1):
    ref = R.reference(pts, leaf, min_points)
    p, c, info = voxel.voxel_filter(pts, leaf, min_points, with_info=True)
    assert c.dtype == np.uint32
    R.check(p, c, (info["n_invalid"], info["n_voxels"], info["n_out"]), ref, leaf)
    index, n, _, _ = voxel.voxel_sums(pts, leaf)
    kept = n >= min_points
    assert [tuple(int(v) for v in k) for k in index[kept]] == ref["keys"]          # keys and order, exactly
    return p, c, ref


def _cloud(dim, n, seed, span=6.0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-span, span, (n, dim)).astype(np.float32)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("leaf", LEAVES)
@pytest.mark.parametrize("min_points", [1, 2, 3])
def test_random_clouds_meet_the_reference(dim, leaf, min_points):
    pts = _cloud(dim, 3001, 10 * dim + min_points, span=12.0 if dim == 2 else 2.5)        # sparse: some voxels hold one point
    p, c, ref = _against_reference(pts, leaf, min_points)
    assert 0 < len(c) < ref["info"][1] + (min_points == 1) and int(c.min()) >= min_points
    if min_points == 1:
        assert int(c.sum()) == 3001


@pytest.mark.parametrize("dim", [2, 3])
def test_negative_coordinates_floor_and_do_not_truncate(dim):
    pts = np.zeros((4, dim), np.float32)
    pts[:, 0] = (-0.1, 0.1, -0.25, -0.26)                      # truncation would give 0, 0, -1, -1
    _, c, ref = _against_reference(pts, 0.25)
    assert [k[0] for k in ref["keys"]] == [-2, -1, 0] and list(c) == [1, 2, 1]
    # float32(-0.3) lies just below -0.3, so it is in voxel -2 of the 0.3 lattice; a voxel's only point comes back
    lone = np.zeros((1, dim), np.float32)
    lone[0, 0] = -0.3
    p, c, ref = _against_reference(lone, 0.3)
    assert ref["keys"][0][0] == -2 and abs(float(p[0, 0]) + 0.3) < 1e-7


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("leaf", LEAVES)
def test_points_exactly_on_lattice_planes(dim, leaf):
    k = np.arange(-9, 10)
    planes = (k * leaf).astype(np.float32)                     # exact for 0.25; the float32 of k * 0.3 otherwise
    pts = np.stack(np.meshgrid(*([planes] * dim), indexing="ij"), -1).reshape(-1, dim)[::3]
    p, c, ref = _against_reference(pts, leaf)
    if leaf == 0.25:
        # a point on a plane belongs to the voxel above it, and a voxel with one point returns that point
        assert ref["keys"] == sorted({tuple(int(v) for v in np.floor(r / 0.25)) for r in pts.astype(np.float64)}, key=lambda t: t[::-1])
        assert int(c.max()) == 1 and np.array_equal(np.sort(p.view(np.uint32) & 0x7FFFFFFF, axis=None),
                                                    np.sort(pts.view(np.uint32) & 0x7FFFFFFF, axis=None))


@pytest.mark.parametrize("dim", [2, 3])
def test_all_points_in_one_voxel_and_every_point_in_its_own(dim):
    rng = np.random.default_rng(5)
    one = (rng.uniform(0.0, 0.2999, (500, dim)) + 3 * 0.3).astype(np.float32)
    p, c, ref = _against_reference(one, 0.3)
    assert list(c) == [500] and ref["keys"] == [(3,) * dim]
    own = (np.stack(np.meshgrid(*([np.arange(-4, 5)] * dim), indexing="ij"), -1).reshape(-1, dim) + 0.37).astype(np.float32)
    rng.shuffle(own)
    p, c, ref = _against_reference(own, 1.0)
    assert len(c) == len(own) and int(c.max()) == 1
    # a single point's centroid is the point: |U| <= 2^21 carries 22 bits of leaf, float32 keeps 24 of the coordinate
    order = np.lexsort(own.T)
    assert np.abs(p - own[order]).max() <= 2.0 ** -22


@pytest.mark.parametrize("dim", [2, 3])
def test_nan_inf_and_the_index_limit(dim):
    pts = _cloud(dim, 64, 3)
    pts[3, 0], pts[10, dim - 1], pts[20, 1] = np.nan, np.inf, -np.inf
    leaf = 0.25
    edge = np.float32(2.0 ** 30 * leaf)                        # i = 2^30 exactly: invalid; the float32 below it: valid
    pts[30, 0], pts[31, 0] = edge, np.nextafter(edge, np.float32(0))
    pts[32, 1], pts[33, 1] = -edge, np.nextafter(-edge, np.float32(0))      # i = -2^30: invalid; the float32 above it: valid
    pts[34, 0] = np.float32(3e38)                             # a quotient far beyond the limit
    p, c, ref = _against_reference(pts, leaf)
    assert ref["info"][0] == 6 and int(c.sum()) == 64 - 6
    # float32 is 16 apart just below 2^28, 64 voxels of 0.25
    assert any(k[0] == 2 ** 30 - 64 for k in ref["keys"]) and any(k[1] == -2 ** 30 + 64 for k in ref["keys"])
    assert all(abs(i) < 2 ** 30 for k in ref["keys"] for i in k)
    allbad = np.full((5, dim), np.nan, np.float32)
    p, c, info = voxel.voxel_filter(allbad, leaf, with_info=True)
    assert p.shape == (0, dim) and c.shape == (0,) and info == dict(n_invalid=5, n_voxels=0, n_out=0)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("min_points", [1, 2])
def test_the_output_does_not_depend_on_the_order_of_the_input(dim, min_points):
    pts = _cloud(dim, 2500, 8, span=2.0)
    pts[17, 0] = np.nan
    want = voxel.voxel_filter(pts, 0.3, min_points, with_info=True)
    for seed in (1, 2, 3):
        got = voxel.voxel_filter(np.random.default_rng(seed).permutation(pts), 0.3, min_points, with_info=True)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2] == want[2]


def test_the_emulated_fma_rounds_once():
    """voxel.fma against exact rational arithmetic, where a product and a sum rounded separately differ from it: sums of
    U of up to 2^50 times a step, beside a centre that cancels most of it or none."""
    rng = np.random.default_rng(2)
    a = rng.integers(-2 ** 50, 2 ** 50, 4000).astype(np.float64)
    b = rng.uniform(1e-9, 1e-6, 4000)
    c = np.where(np.arange(4000) % 2 == 0, rng.uniform(-100.0, 100.0, 4000), -a * b * (1.0 + rng.uniform(-1e-3, 1e-3, 4000)))
    got = voxel.fma(a, b, c)
    exact = np.array([float(Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, exact)
    assert (a * b + c != exact).sum() > 100                    # the inputs do tell the two apart


def test_arguments():
    pts = _cloud(2, 10, 0)
    for leaf in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            voxel.voxel_filter(pts, leaf)
    with pytest.raises(ValueError):
        voxel.voxel_filter(pts, 0.3, min_points=0)
    with pytest.raises(ValueError):
        voxel.voxel_filter(np.zeros((4, 4), np.float32), 0.3)
    assert "oracle" not in open(voxel.__file__).read()
