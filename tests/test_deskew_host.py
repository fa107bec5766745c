"""The host side of the sweep de-skewing (docs/ALGORITHM.md section 2.23): ndt2d/ndt3d_sweep_motion and _motion_twist of the
library, which need no device, and the numpy restatement gtsam_ndt_amd/deskew.py, all against the generic matrix
exponential of tests/deskew_ref.py."""
import math

import numpy as np
import pytest

import deskew_ref as R
from gtsam_ndt_amd import deskew

POSES2 = [(1.0, 2.0, 0.3), (1.3, 1.9, 0.38), (-4.0, 7.5, 3.1), (-4.2, 7.6, -3.1), (0.5, -0.5, -math.pi + 1e-3),
          (0.6, -0.4, math.pi - 1e-3)]
POSES3 = [(1.0, 2.0, 0.5, 0.1, -0.2, 0.3), (1.4, 2.1, 0.45, 0.12, -0.18, 0.42), (0.0, 0.0, 0.0, 0.3, 1.2, -2.0),
          (0.2, -0.1, 0.05, -0.4, -1.2, 3.0), (5.0, 5.0, 1.0, 3.0, 0.7, -3.1), (5.1, 4.8, 1.1, -3.1, 0.6, 3.1)]
MOTIONS2 = [R.MOTION2, (0.25, 0.05, 1e-9), (0.3, -0.2, math.pi - 1e-9), (0.1, 0.4, 1.5 * math.pi)]


def _motion_about(axis, angle, t=(0.5, 0.1, 0.02)):
    return (*t, *R.euler_of(R.rotation_about(axis, angle)))


MOTIONS3 = [R.MOTION3, _motion_about((1.0, 2.0, 3.0), 1e-9), _motion_about((1.0, -2.0, 3.0), 3.0)]


@pytest.fixture(scope="module")
def M(ndt_lib):
    from gtsam_ndt_amd import matcher
    return matcher


@pytest.mark.parametrize("impl", ["library", "numpy"])
def test_sweep_motion_is_the_matrix_product(M, impl):
    f = M.sweep_motion if impl == "library" else deskew.sweep_motion
    for poses in (POSES2, POSES3):
        for prev in poses:
            for cur in poses:
                d = f(prev, cur)
                want = np.linalg.solve(R.pose_matrix(prev), R.pose_matrix(cur))
                assert np.abs(R.pose_matrix(d) - want).max() <= 1e-12, (prev, cur, d)
                if len(prev) == 3:
                    assert -math.pi < d[2] <= math.pi
            z = f(prev, prev)
            assert z == (0.0,) * len(prev), z


def test_sweep_motion_at_gimbal_lock(M):
    """|cos pitch| < 1e-12: roll = 0 is the documented choice, and the pose is still the product's."""
    prev, cur = (0.0,) * 6, (1.0, 2.0, 3.0, 0.4, math.pi / 2, 0.9)
    for f in (M.sweep_motion, deskew.sweep_motion):
        d = f(prev, cur)
        assert d[3] == 0.0 and abs(d[4] - math.pi / 2) < 1e-12
        assert np.abs(R.pose_matrix(d) - R.pose_matrix(cur)).max() <= 1e-12


@pytest.mark.parametrize("impl", ["library", "numpy"])
def test_motion_twist_is_the_logarithm(M, impl):
    f = M.motion_twist if impl == "library" else deskew.motion_twist
    assert f((0.0, 0.0, 0.0)) == (0.0, 0.0, 0.0) and f((0.0,) * 6) == (0.0,) * 6
    for delta in MOTIONS2 + MOTIONS3:
        xi = f(delta)
        assert np.abs(R.expm(R.hat(xi)[None])[0] - R.pose_matrix(delta)).max() <= 1e-12, (delta, xi)
    assert f(MOTIONS2[3])[2] == pytest.approx(-0.5 * math.pi, abs=1e-15)          # wrapped
    assert abs(np.linalg.norm(f(MOTIONS3[2])[3:]) - 3.0) < 1e-12
    assert f(MOTIONS2[1])[2] == 1e-9 and abs(np.linalg.norm(f(MOTIONS3[1])[3:]) - 1e-9) < 1e-15   # the series branch


def test_motion_twist_refuses_what_it_cannot_take(M):
    from gtsam_ndt_amd import _lib
    wide = _motion_about((1.0, 2.0, 3.0), 3.12)
    for delta in (wide, (0.0, 0.0, 0.0, 0.0, 0.0, 3.12), (float("nan"), 0.0, 0.0), (0.0, 0.0, float("inf")),
                  (0.0, 0.0, 0.0, float("nan"), 0.0, 0.0)):
        with pytest.raises(_lib.NdtError) as e:
            M.motion_twist(delta)
        assert e.value.code == _lib.NDT_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            deskew.motion_twist(delta)
    with pytest.raises(_lib.NdtError) as e:
        M.sweep_motion((0.0, float("nan"), 0.0), (0.0, 0.0, 0.0))
    assert e.value.code == _lib.NDT_ERR_INVALID_ARG
    assert len(M.motion_twist(_motion_about((1.0, 2.0, 3.0), 3.09))) == 6


def test_library_and_numpy_twists_agree(M):
    for delta in MOTIONS2 + MOTIONS3:
        assert np.abs(np.array(M.motion_twist(delta)) - np.array(deskew.motion_twist(delta))).max() < 1e-13


@pytest.mark.parametrize("dim", [2, 3])
def test_numpy_restatement_against_the_matrix_exponential(dim):
    """1000 random points within 100 m, fractions in [-0.25, 1.25]: every coordinate within 1e-11 (|p| + |t| + 1) of
    the matrix exponential - a few dozen float64 operations at 2e-16 relative at a scale of 100 m come to about 1e-12."""
    rng = np.random.default_rng(20 + dim)
    pts = rng.uniform(-100.0, 100.0, size=(1000, dim)) / math.sqrt(dim)
    frac = rng.uniform(-0.25, 1.25, size=1000)
    for delta in (MOTIONS2 if dim == 2 else MOTIONS3):
        xi = deskew.motion_twist(delta)
        for ref_frac in (0.0, 0.5, 1.0):
            got = deskew.deskew_points(tuple(pts.T), frac, delta, ref_frac)
            want = R.transform(xi, frac - ref_frac, pts)
            err = np.abs(got - want)
            assert (err <= R.bound(want, pts, delta, rounded=False)).all(), (delta, ref_frac, err.max())


def test_numpy_restatement_identities():
    rng = np.random.default_rng(5)
    pts = rng.uniform(-50.0, 50.0, size=(100, 3))
    pts[3, 0] = -0.0
    frac = rng.uniform(0.0, 1.0, size=100)
    frac[::7] = 1.0
    frac[5], frac[6] = np.nan, np.inf
    same = deskew.deskew_points(tuple(pts.T), frac, (0.0,) * 6, 1.0)
    fin = np.isfinite(frac)
    assert np.array_equal(same[fin].view(np.uint64), pts[fin].view(np.uint64)) and np.isnan(same[~fin]).all()
    got = deskew.deskew_points(tuple(pts.T), frac, R.MOTION3, 1.0)
    at_ref = frac == 1.0
    assert at_ref.sum() >= 10 and np.array_equal(got[at_ref].view(np.uint64), pts[at_ref].view(np.uint64))
    assert np.isnan(got[~fin]).all() and (np.abs(got[fin & ~at_ref] - pts[fin & ~at_ref]).max(axis=1) > 0).all()
    # the range conversions with no motion are the plain conversions
    from gtsam_ndt_amd import synth
    r = rng.uniform(0.0, 40.0, size=64).astype(np.float32)
    r[:3] = (np.nan, np.inf, 0.01)
    x, y = synth.scan_points(r, -1.0, 0.03, 0.05, 30.0)
    p = deskew.polar_to_points(r, -1.0, 0.03, 0.05, 30.0, motion=(0.0, 0.0, 0.0)).astype(np.float32)
    assert np.array_equal(p[:, 0].view(np.uint32), x.view(np.uint32)) and np.array_equal(p[:, 1].view(np.uint32), y.view(np.uint32))
