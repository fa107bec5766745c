"""Self-validation of tests/ndt3d_nb_ref.py, the float64 restatement of the 3D terms over a voxel neighbourhood
(docs/ALGORITHM.md 2.25): neighbourhood 1 is the oracle's evaluate3; at 7 the gradient is the derivative of the
restatement's own score and the Newton Hessian the derivative of its gradient; candidates are taken by index; and the
scene the GPU tests share has no point within 4 float32 ulps of a voxel face and scores 3.5 hits per point at 7."""
import numpy as np
import pytest

from gtsam_ndt_amd import synth3d
from oracle import ndt3d as o

import ndt3d_nb_ref as N


@pytest.fixture(scope="module")
def scene():
    d = synth3d.make_pair3d(n_elev=6, n_azim=256)
    return d, (d["sx"], d["sy"], d["sz"]), o.build_grid3(d["tx"], d["ty"], d["tz"], o.Ndt3Params())


@pytest.mark.parametrize("mode", [0, 1])
def test_neighbourhood_one_is_the_oracle(scene, mode):
    d, S, g = scene
    prm = o.Ndt3Params(hessian_mode=mode)
    for pose in (d["init"], d["pose"]):
        H0, g0, s0, n0 = o.evaluate3(g, *S, pose, prm)
        H1, g1, s1, n1, _ = N.evaluate3_nb(g, *S, pose, prm, 1, mirror32=False)
        assert n1 == n0 > 0
        assert np.abs(H1 - H0).max() <= 1e-12 * np.abs(H0).max()
        assert np.abs(g1 - g0).max() <= 1e-12 * np.abs(g0).max()
        assert abs(s1 - s0) <= 1e-12 * s0


def _stable_poses(scene, count, h):
    """Seeded poses near the generating pose at which no point's own voxel differs between the two ends of any
    central difference of step h; the next seeded pose is taken where one does."""
    d, S, g = scene
    rng = np.random.default_rng(7)
    out = []
    for _ in range(20):
        pose = np.array(d["pose"]) + rng.uniform(-1, 1, 6) * np.array([0.05, 0.05, 0.02, 0.005, 0.005, 0.01])
        base = N.own_voxels3(g, *S, pose, False)
        same = True
        for k in range(6):
            for sgn in (1.0, -1.0):
                e = np.zeros(6); e[k] = sgn * h
                v = N.own_voxels3(g, *S, pose + e, False)
                same = same and np.array_equal(v[2], base[2]) and np.array_equal(v[3], base[3])
        if same:
            out.append(pose)
        if len(out) == count:
            return out
    raise AssertionError("no seeded pose keeps every point in its voxel")


def test_derivatives_at_seven(scene):
    """Tolerances: those of tests/test_oracle3d.py for the single-voxel form (gradient rtol 1e-4 with atol 1e-5 of its
    largest entry; Hessian 1e-5 of its largest entry).  Measured here at step 1e-6: gradient 2e-8 .. 1e-7 of the largest
    entry, Hessian 7e-8 .. 1.5e-6 - the single-voxel form on the same poses gives the same figures."""
    d, S, g = scene
    prm = o.Ndt3Params(hessian_mode=1)
    h = 1e-6
    for pose in _stable_poses(scene, 2, h):
        H, gr = N.evaluate3_nb(g, *S, pose, prm, 7)[:2]
        fd, fdH = np.zeros(6), np.zeros((6, 6))
        for k in range(6):
            e = np.zeros(6); e[k] = h
            p, m = N.evaluate3_nb(g, *S, pose + e, prm, 7), N.evaluate3_nb(g, *S, pose - e, prm, 7)
            fd[k] = -(p[2] - m[2]) / (2 * h)
            fdH[:, k] = (p[1] - m[1]) / (2 * h)
        assert np.allclose(gr, fd, rtol=1e-4, atol=1e-5 * np.abs(gr).max())
        assert np.allclose(H, H.T)
        assert np.abs(H - fdH).max() / np.abs(H).max() < 1e-5
        # the Gauss-Newton form has the same gradient and is not the derivative of it
        Hgn, ggn = N.evaluate3_nb(g, *S, pose, o.Ndt3Params(), 7)[:2]
        assert np.array_equal(ggn, gr) and np.abs(Hgn - fdH).max() / np.abs(H).max() > 1e-3


def test_seven_is_the_sum_of_single_voxel_terms_by_index():
    """A hand-built grid: one valid voxel; a point in a face neighbour scores the term of that voxel, a point in an edge
    or corner neighbour nothing, and a voxel that key - 1 reaches from ix = 0 (the end of the row before) nothing."""
    rng = np.random.default_rng(3)
    prm = o.Ndt3Params()

    def blob(ix, iy, iz):
        return np.array([ix, iy, iz]) + 0.5 + rng.uniform(-0.3, 0.3, size=(8, 3))
    corners = np.array([[0.5, 0.5, 0.5], [8.5, 8.5, 8.5]])        # fix the extent: origin -1, 11 voxels per axis
    pts = np.concatenate([blob(4, 4, 4), corners]).astype(np.float32)
    g = o.build_grid3(pts[:, 0], pts[:, 1], pts[:, 2], prm)
    assert tuple(g.o) == (-1.0, -1.0, -1.0) and g.dims == (11, 11, 11) and g.n_valid == 1
    # a build leaves the last column empty; a grid that grew by updates need not: the same record once more at
    # index (W - 1, 3, 5), which is the cloud's (9, 2, 4)
    k, k2 = (5 * 11 + 5) * 11 + 5, (5 * 11 + 3) * 11 + 10
    g.valid[k2] = True
    g.mean[k2] = g.mean[k] + np.array([5.0, -2.0, 0.0])
    g.icov[k2] = g.icov[k]
    zero = (0.0,) * 6

    def ev(p, nb):
        p = np.asarray(p, np.float64)[None, :]
        return N.evaluate3_nb(g, p[:, 0], p[:, 1], p[:, 2], zero, prm, nb)
    for dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
        p = np.array([4.5, 4.5, 4.5]) + np.array(dx)
        assert ev(p, 1)[3] == 0 and ev(p, 7)[3] == 1
        k = (5 * g.dims[1] + 5) * g.dims[0] + 5                    # voxel (4, 4, 4) of the cloud is index 5 per axis
        q = p - g.mean[k]
        ic = g.icov[k]
        C = np.array([[ic[0], ic[1], ic[2]], [ic[1], ic[3], ic[4]], [ic[2], ic[4], ic[5]]])
        assert abs(ev(p, 7)[2] - prm.d1 * np.exp(-0.5 * prm.d2 * q @ C @ q)) <= 1e-15
    for dx in ((1, 1, 0), (0, 1, -1), (1, 1, 1), (-1, 1, -1)):
        assert ev(np.array([4.5, 4.5, 4.5]) + np.array(dx), 7)[3] == 0
    # the valid voxel at the cloud's (9, 2, 4) is index (10, 3, 5) = W - 1: key + 1 is (0, 4, 5), a point there is at -0.5
    assert g.dims[0] == 11
    assert ev((-0.5, 3.5, 4.5), 7)[3] == 0 and ev((8.5, 2.5, 4.5), 7)[3] == 1
    # outside the grid, a quarter cell past the face next to a valid voxel, and a NaN point: nothing
    assert ev((10.25, 2.5, 4.5), 7)[3] == 0 and ev((np.nan, 2.5, 4.5), 7)[3] == 0


def test_the_gpu_scene_has_no_border_points_and_many_neighbours(scene):
    """What tests/test_gpu_neighbourhood3d.py assumes of the seeded scene, checked where no device is needed: at most 3
    points within 4 float32 ulps of a voxel face (measured: 0), and over 1.5 hits at 7 per hit at 1 (measured: 3.5)."""
    d, S, g = scene
    prm = o.Ndt3Params()
    for pose in (d["init"], d["pose"]):
        r1 = N.evaluate3_nb(g, *S, pose, prm, 1, mirror32=True)
        r7 = N.evaluate3_nb(g, *S, pose, prm, 7, mirror32=True)
        assert r7[4] <= 3
        assert r7[3] > 1.5 * r1[3] > 0
        # the float32 image moves no point across a face here: the hit counts are those of the float64 image
        assert r7[3] == N.evaluate3_nb(g, *S, pose, prm, 7, mirror32=False)[3]


def test_align_is_the_oracles_loop():
    """16 x 256 points: the smallest scene of this generator on which both neighbourhoods converge."""
    d = synth3d.make_pair3d(n_elev=16, n_azim=256)
    S = (d["sx"], d["sy"], d["sz"])
    prm = o.Ndt3Params()
    g = o.build_grid3(d["tx"], d["ty"], d["tz"], prm)
    ref = o.align3(g, *S, d["init"], prm)
    r1 = N.align3_nb(g, *S, d["init"], prm, 1)
    assert (r1["status"], r1["iterations"], r1["n_hit"]) == (ref["status"], ref["iterations"], ref["n_hit"]) and ref["status"] == 0
    assert np.abs(np.array(r1["pose"]) - np.array(ref["pose"])).max() < 1e-9
    trace = []
    r7 = N.align3_nb(g, *S, d["init"], prm, 7, trace=trace)
    assert r7["status"] == 0 and len(trace) == r7["iterations"] and r7["n_hit"] > 1.5 * r1["n_hit"]
    assert np.abs(np.array(r7["pose"]) - np.array(r1["pose"])).max() > 1e-6        # another objective, another optimum
