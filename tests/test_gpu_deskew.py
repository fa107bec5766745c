"""Sweep de-skewing on the device (docs/ALGORITHM.md section 2.23): ndt2d_polar_to_points_deskew_dev,
ndt3d_range_image_to_points_deskew_dev and ndt2d/ndt3d_deskew_points_dev - the identities bit for bit, every entry within
half a float32 ulp (+ 1e-11 relative) of the generic matrix exponential of tests/deskew_ref.py, in place, in stream order,
and end to end: the sweep of a moving sensor aligns like a static scan once de-skewed, and does not as it came."""
import math

import numpy as np
import pytest

import deskew_ref as R
from gtsam_ndt_amd import synth, synth3d

pytestmark = pytest.mark.gpu

KBLOCK = 256                                    # workgroup size of the streaming kernels (csrc/ndt2d_kernels.hpp)
RMIN, RMAX = 0.05, 100.0
SLEEP_CYCLES = 200_000_000                      # ~0.1 s of torch.cuda._sleep on the producer stream
TINY2 = (0.25, 0.05, 1e-9)                      # rotations in the power-series branch ...
TINY3 = (0.5, 0.1, 0.02, *R.euler_of(R.rotation_about((1.0, 2.0, 3.0), 1e-9)))
WIDE3 = (0.5, 0.1, 0.02, *R.euler_of(R.rotation_about((1.0, -2.0, 3.0), 3.0)))      # ... and close to the 3.1 rad limit
EL16 = np.deg2rad(np.linspace(-24.0, 20.0, 16))


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _ranges(shape, seed):
    """Ranges up to 100 m with a NaN, a +inf, a too-near and a too-far value (as many as fit)."""
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.5, 100.0, size=shape).astype(np.float32)
    flat = r.reshape(-1)
    for k, v in zip(range(0, flat.size, max(1, flat.size // 4)), (np.nan, np.inf, 0.01, 500.0)):
        flat[k] = v
    return r


def _valid(r):
    return np.isfinite(r) & (r >= np.float32(RMIN)) & (r <= np.float32(RMAX))


def _points(n, dim, seed):
    rng = np.random.default_rng(seed)
    p = (rng.uniform(-100.0, 100.0, size=(n, dim)) / math.sqrt(dim)).astype(np.float32)
    f = rng.uniform(-0.25, 1.25, size=n).astype(np.float32)
    return p, f


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ 4: motion = 0
@pytest.mark.parametrize("n", [1, KBLOCK + 1, 1440])
def test_no_motion_is_the_plain_conversion_2d(gpu_lib, n):
    from gtsam_ndt_amd.matcher import polar_to_points
    r = _ranges(n, n)
    d = _cuda(r)
    plain = polar_to_points(d, -math.pi, 2.0 * math.pi / n, RMIN, RMAX)
    for ref_frac in (1.0, 0.0, 0.37):
        got = polar_to_points(d, -math.pi, 2.0 * math.pi / n, RMIN, RMAX, motion=(0.0, 0.0, 0.0), ref_frac=ref_frac)
        for g, p in zip(got, plain):
            assert np.array_equal(_bits(g), _bits(p))
            assert np.array_equal(np.isnan(g.cpu().numpy()), ~_valid(r))


@pytest.mark.parametrize("shape", [(3, 70), (16, 256)])
def test_no_motion_is_the_plain_conversion_3d(gpu_lib, shape):
    from gtsam_ndt_amd.matcher import range_image_to_points
    r = _ranges(shape, shape[1])
    d = _cuda(r)
    el = np.deg2rad(np.linspace(-24.0, 20.0, shape[0]))
    inc = 2.0 * math.pi / shape[1]
    plain = range_image_to_points(d, el, 0.5 * inc, inc, RMIN, RMAX)
    for ref_frac in (1.0, 0.37):
        got = range_image_to_points(d, el, 0.5 * inc, inc, RMIN, RMAX, motion=(0.0,) * 6, ref_frac=ref_frac)
        for g, p in zip(got, plain):
            assert np.array_equal(_bits(g), _bits(p))
            assert np.array_equal(np.isnan(g.cpu().numpy()), ~_valid(r).reshape(-1))


@pytest.mark.parametrize("dim", [2, 3])
def test_no_motion_returns_the_points_bits(gpu_lib, dim):
    from gtsam_ndt_amd.matcher import deskew_points
    p, f = _points(1000, dim, 40 + dim)
    p[5] = np.nan                                # a NaN point, a half-NaN point, a signed zero
    p[6, 0] = np.nan
    p[7, 1] = -0.0
    got = deskew_points(tuple(_cuda(p[:, k]) for k in range(dim)), _cuda(f), (0.0,) * (3 * dim - 3), 0.5)
    for k in range(dim):
        assert np.array_equal(_bits(got[k]), np.ascontiguousarray(p[:, k]).view(np.uint32))


# ------------------------------------------------------------------------------------------------ 5: s == s_ref
@pytest.mark.parametrize("dim", [2, 3])
def test_a_point_at_the_reference_fraction_is_untouched(gpu_lib, dim):
    from gtsam_ndt_amd.matcher import deskew_points
    p, f = _points(1000, dim, 50 + dim)
    f[::3] = 1.0
    f[1], f[2] = np.nan, np.inf
    p[3, 0] = -0.0
    p[6] = np.nan
    got = [g.cpu().numpy() for g in deskew_points(tuple(_cuda(p[:, k]) for k in range(dim)), _cuda(f),
                                                  R.MOTION2 if dim == 2 else R.MOTION3, 1.0)]
    at_ref = f == 1.0
    assert at_ref.sum() > 300
    moved = np.isfinite(f) & ~at_ref & np.isfinite(p).all(axis=1)
    for k in range(dim):
        assert np.array_equal(got[k][at_ref].view(np.uint32), p[at_ref, k].view(np.uint32))
        assert np.isnan(got[k][~np.isfinite(f)]).all()
    assert (np.stack(got, axis=1)[moved] != p[moved]).any(axis=1).mean() > 0.99     # (a fraction within 1e-5 of 1 moves a point by less than a float32 ulp)


# ------------------------------------------------------------------------------------------------ 6: accuracy
def _check(got, want, pts, delta, ok):
    got = np.stack([g.cpu().numpy() for g in got], axis=1)
    assert np.array_equal(np.isnan(got).any(axis=1), ~ok) and np.array_equal(np.isnan(got).all(axis=1), ~ok)
    err = np.abs(got[ok].astype(np.float64) - want[ok])
    lim = R.bound(want[ok], pts[ok], delta)
    print(f"delta {delta}: worst error / bound {np.max(err / lim):.3f}")
    assert (err <= lim).all()


@pytest.mark.parametrize("delta", [R.MOTION2, TINY2])
def test_polar_conversion_against_the_matrix_exponential(gpu_lib, delta):
    from gtsam_ndt_amd.matcher import motion_twist, polar_to_points
    n = 1440
    r = _ranges(n, 6)
    a0, inc = -math.pi, 2.0 * math.pi / n
    ang = a0 + inc * np.arange(n)
    pts = np.stack([r.astype(np.float64) * np.cos(ang), r.astype(np.float64) * np.sin(ang)], axis=1)
    s = -0.25 + (1.5 / n) * np.arange(n)
    xi = motion_twist(delta)
    ok = _valid(r)
    for ref_frac in (0.0, 1.0, 0.5):
        got = polar_to_points(_cuda(r), a0, inc, RMIN, RMAX, motion=delta, frac=(-0.25, 1.5 / n), ref_frac=ref_frac)
        want = np.full_like(pts, np.nan)
        want[ok] = R.transform(xi, s[ok] - ref_frac, pts[ok])
        _check(got, want, pts, delta, ok)


@pytest.mark.parametrize("delta", [R.MOTION3, TINY3, WIDE3])
def test_range_image_conversion_against_the_matrix_exponential(gpu_lib, delta):
    from gtsam_ndt_amd.matcher import motion_twist, range_image_to_points
    ne, na = 16, 256
    r = _ranges((ne, na), 7)
    inc = 2.0 * math.pi / na
    E, A = np.meshgrid(EL16, 0.5 * inc + inc * np.arange(na), indexing="ij")
    r64 = r.astype(np.float64)
    pts = np.stack([r64 * (np.cos(E) * np.cos(A)), r64 * (np.cos(E) * np.sin(A)), r64 * np.sin(E)], axis=-1).reshape(-1, 3)
    s = np.broadcast_to((-0.25 + (1.5 / na) * np.arange(na))[None, :], (ne, na)).reshape(-1)
    xi = motion_twist(delta)
    ok = _valid(r).reshape(-1)
    for ref_frac in (0.0, 1.0, 0.5):
        got = range_image_to_points(_cuda(r), EL16, 0.5 * inc, inc, RMIN, RMAX, motion=delta, frac=(-0.25, 1.5 / na),
                                    ref_frac=ref_frac)
        want = np.full_like(pts, np.nan)
        want[ok] = R.transform(xi, s[ok] - ref_frac, pts[ok])
        _check(got, want, pts, delta, ok)


@pytest.mark.parametrize("delta", [R.MOTION2, TINY2, R.MOTION3, TINY3, WIDE3])
def test_point_entries_against_the_matrix_exponential(gpu_lib, delta):
    from gtsam_ndt_amd.matcher import deskew_points, motion_twist
    dim = 2 if len(delta) == 3 else 3
    p, f = _points(1000, dim, 60 + dim)
    f[4] = np.nan
    xi = motion_twist(delta)
    ok = np.isfinite(f)
    pts = p.astype(np.float64)
    for ref_frac in (0.0, 1.0, 0.5):
        got = deskew_points(tuple(_cuda(p[:, k]) for k in range(dim)), _cuda(f), delta, ref_frac)
        want = np.full_like(pts, np.nan)
        want[ok] = R.transform(xi, f[ok].astype(np.float64) - ref_frac, pts[ok])
        _check(got, want, pts, delta, ok)


# ------------------------------------------------------------------------------------------------ 7: aliasing
@pytest.mark.parametrize("dim", [2, 3])
def test_in_place_equals_out_of_place(gpu_lib, dim):
    from gtsam_ndt_amd.matcher import deskew_points
    p, f = _points(1000, dim, 70 + dim)
    delta = R.MOTION2 if dim == 2 else R.MOTION3
    coords = tuple(_cuda(p[:, k]) for k in range(dim))
    want = deskew_points(coords, _cuda(f), delta, 1.0)
    assert all(w.data_ptr() != c.data_ptr() for w, c in zip(want, coords))
    got = deskew_points(coords, _cuda(f), delta, 1.0, out=coords)
    for g, c, w, k in zip(got, coords, want, range(dim)):
        assert g is c and np.array_equal(_bits(c), _bits(w)) and not np.array_equal(_bits(c), p[:, k].copy().view(np.uint32))


# ------------------------------------------------------------------------------------------------ 8: stream order
def _target2d(sc):
    r0, a0, da = synth.lidar_scan2d(sc, (8.0, 10.0, 0.0), n_beams=7200, seed=100)
    x0, y0 = synth.scan_points(r0, a0, da)
    ok = ~np.isnan(x0)
    return (x0[ok] + np.float32(8.0)).astype(np.float32), (y0[ok] + np.float32(10.0)).astype(np.float32)


@pytest.fixture(scope="module")
def sweep2():
    """The 2D end-to-end case: the room, the target built from the 7200-beam scan at (8, 10, 0), and the 1440-beam sweep
    that starts at (9.5, 10.8, 0.1) and moves by MOTION2 while it turns."""
    from gtsam_ndt_amd import deskew
    sc = synth.room_scene(4242, 30.0)
    tx, ty = _target2d(sc)
    r, a0, inc, end = R.sweep2d(sc, (9.5, 10.8, 0.1), deskew.motion_twist(R.MOTION2), 1440)
    return dict(tx=tx, ty=ty, r=r, a0=a0, inc=inc, end=end, guess=(end[0] + 0.05, end[1] - 0.04, end[2] + 0.01))


def test_conversion_behind_a_late_producer(gpu_lib, sweep2):
    import torch
    from gtsam_ndt_amd.matcher import NdtMatcher2D, polar_to_points
    w = sweep2
    ranges = _cuda(w["r"])
    with NdtMatcher2D() as m:
        m.set_target(w["tx"], w["ty"])
        dx, dy = polar_to_points(ranges, w["a0"], w["inc"], 0.05, 30.0, motion=R.MOTION2)
        torch.cuda.synchronize()
        want = m.align(dx, dy, w["guess"])                    # everything complete: the reference run
        assert want.status == 0
        del dx, dy
        junk = [torch.full((ranges.numel(),), float("nan"), dtype=torch.float32, device="cuda") for _ in range(4)]
        torch.cuda.synchronize()
        del junk                                              # NaN in the blocks the next torch.empty calls are handed
        torch.cuda._sleep(SLEEP_CYCLES)                       # the producer stream is busy ...
        late = ranges + 0.0                                   # ... so the ranges do not exist yet
        dx, dy = polar_to_points(late, w["a0"], w["inc"], 0.05, 30.0, motion=R.MOTION2)
        got = m.align(dx, dy, w["guess"])                     # wait_stream inside; no host synchronisation in between
        assert got.status == 0 and got.pose == want.pose and got.n_hit == want.n_hit


# ------------------------------------------------------------------------------------------------ 9: end to end, 2D
def test_moving_sweep_aligns_once_deskewed_2d(gpu_lib, sweep2):
    """float64 oracle on the CPU: raw sweep 0.026 m / 0.030 rad off the end pose, de-skewed 8e-4 m / 9e-5 rad, a static scan
    from the end pose 7e-4 m / 1e-5 rad."""
    from gtsam_ndt_amd.matcher import NdtMatcher2D, polar_to_points
    from oracle import ndt2d as o
    w = sweep2
    end = np.array(w["end"])
    ranges = _cuda(w["r"])
    with NdtMatcher2D() as m:
        m.set_target(w["tx"], w["ty"])
        dx, dy = polar_to_points(ranges, w["a0"], w["inc"], 0.05, 30.0, motion=R.MOTION2, ref_frac=1.0)
        got = m.align(dx, dy, w["guess"])
        rx, ry = polar_to_points(ranges, w["a0"], w["inc"], 0.05, 30.0)
        raw = m.align(rx, ry, w["guess"])
    x, y = dx.cpu().numpy(), dy.cpu().numpy()
    ok = ~np.isnan(x)
    prm = o.NdtParams()
    ref = o.align(o.build_grid(w["tx"], w["ty"], prm), x[ok], y[ok], w["guess"], prm)
    e, eo, er = np.abs(np.array(got.pose) - end), np.abs(np.array(got.pose) - np.array(ref["pose"])), np.abs(np.array(raw.pose) - end)
    print(f"de-skewed {e}, against the oracle {eo}, raw {er} (status {raw.status})")
    assert got.status == 0 and e.max() < 5e-3
    assert ref["status"] == 0 and eo.max() < 1e-4
    assert er.max() > 5e-3


# ------------------------------------------------------------------------------------------------ 10: end to end, 3D
def test_moving_sweep_aligns_once_deskewed_3d(gpu_lib):
    """A 16 x 256 sweep that starts at (0.6, 0.3, 0.02, 0.004, -0.006, 0.05) and moves by MOTION3, against the 32 x 1024
    static scan from the zero pose.  float64 oracle on the CPU (oracle.ndt3d.align3, same guess), error against the end
    pose: raw sweep 0.0605 m / 0.0091 rad (3x the bound), de-skewed 0.0006 m / 0.00016 rad, a static scan from the end
    pose 0.0011 m / 0.00018 rad."""
    from gtsam_ndt_amd import deskew
    from gtsam_ndt_amd.matcher import NdtMatcher3D, range_image_to_points
    t = synth3d.lidar_scan(101, (0.0,) * 6, 32, 1024).astype(np.float32)
    rng, el, az0, inc, end = R.sweep3d((0.6, 0.3, 0.02, 0.004, -0.006, 0.05), deskew.motion_twist(R.MOTION3), 16, 256)
    guess = tuple(np.array(end) + np.array([0.05, -0.04, 0.01, 0.002, -0.002, 0.01]))
    d = _cuda(rng)
    with NdtMatcher3D() as m:
        m.set_target(*(np.ascontiguousarray(t[:, k]) for k in range(3)))
        got = m.align(*range_image_to_points(d, el, az0, inc, 0.05, 100.0, motion=R.MOTION3), guess)
        raw = m.align(*range_image_to_points(d, el, az0, inc, 0.05, 100.0), guess)
    e, er = np.abs(np.array(got.pose) - np.array(end)), np.abs(np.array(raw.pose) - np.array(end))
    print(f"de-skewed {e}, raw {er} (status {raw.status})")
    assert got.status == 0 and e[:3].max() < 0.02 and e[3:].max() < 3e-3
    assert er[:3].max() > 0.02 or er[3:].max() > 3e-3
