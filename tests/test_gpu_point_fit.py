"""ndt2d/ndt3d_fit_points*: per-point m and class against tests/point_fit_ref.py (float64, fed the device's own
records), on the committed fixtures with NaN / inf, far, ring and displaced points injected.

1. A pose without rotation and with float32 translations: the device's image point is one float32 add per axis, numpy
   float32 reproduces it and the key exactly.  invalid / miss / hit are equal at EVERY point; |m_dev - m_ref| <=
   K 2^-24 M_abs per hit (K = 8 in 2D, 10 in 3D; point_fit_ref states the count); fit / misfit equal wherever m_ref is
   further than that from max_m, and at most 1 % of the hits may be excused that way.
2. Rotated poses (the fixture's final pose, one with |theta| > 2, and in 3D the scan seen from a frame rolled 0.7 and
   pitched -0.5 rad): the same with the image-point uncertainty added
   (point_fit_ref), points whose cell coordinate is within it of an integer excused under the same 1 % cap; and the tie
   to the existing path for one grid and 3D: n_misfit + n_fit EQUALS evaluate(...).n_hit, and sum d1 exp(-d2 / 2 m_i)
   over the hits, added in float64 from the returned m, is within 2e-5 relative of its score (the project's standing
   score tolerance, VERDICT row a5)."""
import numpy as np
import pytest

import point_fit_cases as PC
import point_fit_ref as F

pytestmark = pytest.mark.gpu

CONFIGS = [(2, 1), (2, 4), (3, 1)]
N = 4500            # five tiles of 1024, the last one partial


@pytest.fixture(scope="module")
def scenes(gpu_lib):
    out = {}
    for dim, ng in CONFIGS:
        m = PC.matcher(dim, ng)
        out[dim, ng] = (m, F.records_of(m), PC.fixture(dim))
    yield out
    for m, _, _ in out.values():
        m.close()


def _fit_both_ways(m, coords, pose, max_m):
    """Host arrays and device tensors: the same bytes."""
    host = m.fit_points(*coords, pose, max_m)
    d = m.fit_points(*PC.dev(coords), pose, max_m)
    assert isinstance(host.m, np.ndarray) and host.m.dtype == np.float32 and host.cls.dtype == np.uint8
    dm, dc = d.m.cpu().numpy(), d.cls.cpu().numpy()
    assert host.m.tobytes() == dm.tobytes() and host.cls.tobytes() == dc.tobytes()
    assert PC.fit_tuple(host) == PC.fit_tuple(d) and host.n_selected == 0
    c = F.counts(host.cls)
    assert (host.n_invalid, host.n_miss, host.n_misfit, host.n_fit) == (c["n_invalid"], c["n_miss"], c["n_misfit"], c["n_fit"])
    assert host.n_invalid + host.n_miss + host.n_misfit + host.n_fit == len(coords[0])
    return host


def _check(ref, got, max_m, what):
    fig, fails = F.compare(ref, got.m, got.cls, max_m)
    print(f"{what}: {fig} counts {PC.fit_tuple(got)}")
    assert not fails, (what, fails, fig)
    return fig


@pytest.mark.parametrize("dim,ng", CONFIGS)
def test_exact_image_pose(scenes, dim, ng):
    m, rec, fx = scenes[dim, ng]
    pose, max_m = PC.EXACT_POSE[dim], PC.MAX_M[dim]
    coords, inj = PC.mixed_scan(rec, fx["source"], pose, N)
    ref = F.fit_ref(rec, coords, pose, max_m, exact=True)
    assert not ref["near"].any()
    got = _fit_both_ways(m, coords, pose, max_m)
    assert np.array_equal(np.minimum(got.cls, 2), np.minimum(ref["cls"], 2))          # invalid / miss / hit: every point
    fig = _check(ref, got, max_m, f"exact pose dim {dim} ngrid {ng}")
    assert fig["n_hit"] > 1000 and got.n_fit > 0 and got.n_misfit > 0
    assert np.all(got.cls[inj["bad"]] == F.INVALID) and np.all(got.cls[inj["far"]] == F.MISS)
    assert np.all(got.cls[inj["ring"]] == F.MISS)
    assert np.all((got.cls[inj["displaced"]] == F.MISS) | (got.cls[inj["displaced"]] == F.MISFIT))


@pytest.mark.parametrize("which", ["final", "far"])
@pytest.mark.parametrize("dim,ng", CONFIGS)
def test_rotated_pose(scenes, dim, ng, which):
    m, rec, fx = scenes[dim, ng]
    pose = fx["final_pose"] if which == "final" else PC.far_pose(dim, fx["final_pose"])
    _rotated_pose(m, rec, fx["source"], pose, dim, ng, which)


def test_steep_pose_3d(scenes):
    """Roll 0.7, pitch -0.5, yaw 2.1 (point_fit_cases.steep_scene): every entry of R away from 0 and 1, the same bound."""
    m, rec, fx = scenes[3, 1]
    source, pose = PC.steep_scene(fx)
    _rotated_pose(m, rec, source, pose, 3, 1, "steep")


def _rotated_pose(m, rec, source, pose, dim, ng, which):
    max_m = PC.MAX_M[dim]
    coords, inj = PC.mixed_scan(rec, source, pose, N)
    ref = F.fit_ref(rec, coords, pose, max_m)
    got = _fit_both_ways(m, coords, pose, max_m)
    fig = _check(ref, got, max_m, f"{which} pose dim {dim} ngrid {ng}")
    assert fig["n_hit"] > 300
    assert np.all(got.cls[inj["bad"]] == F.INVALID) and np.all(got.cls[inj["far"]] == F.MISS)
    if ng == 1:
        # the tie to the existing device path, on the finite points of the scan
        fin = ref["finite"]
        sub = tuple(c[fin] for c in coords)
        _, _, score, n_hit = m.evaluate(*sub, pose)
        assert got.n_misfit + got.n_fit == n_hit
        hit = got.cls >= F.MISFIT
        d1, d2 = float(m.params.d1), float(m.params.d2)
        mine = float(np.sum(d1 * np.exp(-0.5 * d2 * got.m[hit].astype(np.float64))))
        print(f"score from m {mine!r} evaluate {score!r} rel {abs(mine - score) / abs(score):.3e}")
        assert abs(mine - score) <= 2e-5 * abs(score)


@pytest.mark.parametrize("dim,ng", CONFIGS)
def test_infinite_threshold_and_empty_grid(scenes, dim, ng):
    """max_m = +inf: every hit fits.  A reserved grid without a point: every finite point is a miss, and no error."""
    m, rec, fx = scenes[dim, ng]
    pose = fx["final_pose"]
    coords, _ = PC.mixed_scan(rec, fx["source"], pose, 1500)
    got = m.fit_points(*coords, pose, float("inf"))
    ref = F.fit_ref(rec, coords, pose, PC.MAX_M[dim])
    assert got.n_misfit == 0 and got.n_fit > 0 and got.n_invalid == int((~ref["finite"]).sum())
    zero = m.fit_points(*coords, pose, 0.0)
    assert zero.n_fit + zero.n_misfit == got.n_fit and np.array_equal(zero.cls >= F.MISFIT, got.cls >= F.MISFIT)
    assert np.all(zero.m[zero.cls == F.FIT] <= 0.0)
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D
    with (NdtMatcher2D(overlap_grids=ng) if dim == 2 else NdtMatcher3D()) as e:
        if dim == 2:
            e.reserve_target(-20.0, -20.0, 20.0, 20.0)
        else:
            e.reserve_target((-20.0, -20.0, -5.0), (20.0, 20.0, 5.0))
        r = e.fit_points(*coords, pose, PC.MAX_M[dim])
        assert (r.n_invalid, r.n_miss, r.n_misfit, r.n_fit) == (got.n_invalid, len(coords[0]) - got.n_invalid, 0, 0)
        assert np.all(np.isposinf(r.m[r.cls == F.MISS])) and np.all(np.isnan(r.m[r.cls == F.INVALID]))
