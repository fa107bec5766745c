"""ndt3d_remove_target_points(_dev): taking a scan out of a voxel submap is the exact inverse of adding it.

32 x 1024-beam scans in the reserved box of tests/test_gpu_scan_sequence3d.py: the voxels round the sensor hold more than
1 024 points per 4 x 4 x 4 tile, so shared tiles and their slabs are exercised.  Expectations come from the library's own
add path and from numpy voxel counts of the points that should remain - never from the removal itself."""
import numpy as np
import pytest

from gtsam_ndt_amd import synth3d
from handle_life import moved3d as _world     # ndt3d_add_target_points_dev's float32 restatement

pytestmark = pytest.mark.gpu

POSES = [(0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.6, 0.3, 0.02, 0.004, -0.006, 0.05), (1.3, 0.5, -0.01, -0.005, 0.004, 0.11),
         (1.9, 1.1, 0.03, 0.006, 0.002, 0.16)]
LO, HI = (-22.0, -22.0, -3.0), (22.0, 22.0, 6.0)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _state(m):
    gi = m.grid_info()
    return {"map": m.save_map().tobytes(), "grid": m.grid(),
            "info": (gi.width, gi.height, gi.depth, gi.ox, gi.oy, gi.oz, gi.n_valid)}


def _assert_same_state(got, want):
    assert got["info"] == want["info"]
    for u, v in zip(got["grid"], want["grid"]):
        np.testing.assert_array_equal(u, v)
    assert got["map"] == want["map"]


@pytest.fixture(scope="module")
def M(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    return NdtMatcher3D


@pytest.fixture(scope="module")
def scans(gpu_lib):
    out = []
    for k, pose in enumerate(POSES):
        p = synth3d.lidar_scan(200 + k, pose, n_elev=32, n_azim=1024, sigma=0.02)
        xyz = [np.ascontiguousarray(p[:, a], dtype=np.float32) for a in range(3)]
        for c in xyz:
            c[[5, 9000, 32767]] = np.nan                             # beams without a return
        est = tuple(np.array(pose) + np.array([0.004, -0.003, 0.002, 0.0003, -0.0002, 0.0005]))     # what an alignment returns
        out.append((xyz, est))
    return out


def test_remove_is_the_exact_inverse_of_add_3d(M, scans):
    (s0, p0), (s1, p1), (s2, p2), (s3, p3) = scans
    d0, d1, d2 = ([_dev(c) for c in s] for s in (s0, s1, s2))
    with M() as m, M() as ref:
        m.reserve_target(LO, HI)
        ref.reserve_target(LO, HI)
        outs = [ref.add_target_points(*d0, pose=p0), ref.add_target_points(*d2, pose=p2)]
        assert m.add_target_points(*d0, pose=p0) == outs[0]
        out1 = m.add_target_points(*d1, pose=p1)
        assert m.add_target_points(*d2, pose=p2) == outs[1]
        with_s1 = m.grid()[0].astype(np.int64).sum()
        assert m.remove_target_points(*d1, pose=p1) == out1 >= 3      # the NaN beams count as outside, both ways
        st = _state(m)
        _assert_same_state(st, _state(ref))
        guess = tuple(np.array(POSES[3]) + np.array([0.05, -0.04, 0.01, 0.002, -0.002, 0.01]))
        a, b = m.align(*[_dev(c) for c in s3], guess), ref.align(*[_dev(c) for c in s3], guess)
        assert a.status == 0 and a.pose == b.pose and a.iterations == b.iterations and a.score == b.score
    # numpy voxel counts of what should remain; the tiles round the sensor were shared
    count = st["grid"][0].astype(np.int64)
    assert with_s1 - count.sum() == s1[0].size - out1 > 30000
    w, h, d, ox, oy, oz = st["info"][:6]
    P = np.concatenate([np.stack(_world(*s0, p0), axis=1), np.stack(_world(*s2, p2), axis=1)])
    P = P[~np.isnan(P[:, 0])]
    idx = np.floor(P - np.array([ox, oy, oz], np.float32)).astype(np.int64)          # (1 m voxels: inv_cell = 1)
    inside = np.all((idx >= 0) & (idx < np.array([w, h, d])), axis=1)
    key = (idx[:, 2] * h + idx[:, 1]) * w + idx[:, 0]
    want = np.bincount(key[inside], minlength=w * h * d)
    np.testing.assert_array_equal(count, want)
    tiles = np.zeros(((d + 3) // 4, (h + 3) // 4, (w + 3) // 4), np.int64)
    P1 = np.stack(_world(*s1, p1), axis=1)[~np.isnan(s1[0])]
    i1 = np.floor(P1 - np.array([ox, oy, oz], np.float32)).astype(np.int64)
    i1 = i1[np.all((i1 >= 0) & (i1 < np.array([w, h, d])), axis=1)]
    np.add.at(tiles, (i1[:, 2] // 4, i1[:, 1] // 4, i1[:, 0] // 4), 1)
    assert tiles.max() > 1024                                        # the removed scan did put shared tiles to work


def test_add_and_remove_at_a_steep_pose_3d(M, scans):
    """A scan seen from a sensor frame rolled 0.7 and pitched -0.5 rad (every other pose here stays below 0.006): the
    scan re-expressed, s' = Q' s with Q = R(pose)' R(steep), lands where the original does.  Added on the device at the
    steep pose, the grid is the one built from the host-transformed points (_world: numpy's R, float32); removed again,
    the submap is bit for bit what it was."""
    (s0, p0), (s1, p1) = scans[0], scans[1]
    steep = (0.7, -0.5, 2.1)
    Q = synth3d.rotation(*p1[3:]).T @ synth3d.rotation(*steep)
    P = np.stack(s1, axis=1).astype(np.float64) @ Q
    t1 = [np.ascontiguousarray(P[:, a].astype(np.float32)) for a in range(3)]
    pt = tuple(p1[:3]) + steep
    w = _world(*t1, pt)
    seen = ~np.isnan(s1[0])
    assert np.abs(np.stack(w, 1)[seen] - np.stack(_world(*s1, p1), 1)[seen]).max() < 1e-4          # the same place
    d0, dt = [_dev(c) for c in s0], [_dev(c) for c in t1]
    with M() as m, M() as ref, M() as base:
        for h in (m, ref, base):
            h.reserve_target(LO, HI)
            h.add_target_points(*d0, pose=p0)
        before = _state(base)
        out = m.add_target_points(*dt, pose=pt)
        assert ref.add_target_points(*w) == out >= 3                  # host arrays, already in the map frame
        st = _state(m)
        _assert_same_state(st, _state(ref))
        assert st["grid"][0].astype(np.int64).sum() - before["grid"][0].astype(np.int64).sum() == t1[0].size - out > 30000
        assert m.remove_target_points(*dt, pose=pt) == out
        _assert_same_state(_state(m), before)


def test_host_entry_point_and_remove_everything_3d(M, scans):
    (s0, p0), (s1, p1) = scans[0], scans[1]
    w0, w1 = _world(*s0, p0), _world(*s1, p1)
    with M() as m, M() as ref, M() as fresh:
        fresh.reserve_target(LO, HI)
        ref.reserve_target(LO, HI)
        out0 = ref.add_target_points(*w0)
        m.reserve_target(LO, HI)
        assert m.add_target_points(*w0) == out0
        out1 = m.add_target_points(*w1)
        assert m.remove_target_points(*w1) == out1                   # host arrays, no pose
        _assert_same_state(_state(m), _state(ref))
        assert m.grid_info().n_valid > 100
        # everything removed: a fresh reserve of the same box
        assert m.remove_target_points(*[_dev(c) for c in s0], pose=p0) == out0
        assert m.grid_info().n_valid == 0
        _assert_same_state(_state(m), _state(fresh))
        assert m.align(*s1, POSES[1]).status == 4                    # NDT_TOO_FEW_CELLS
        with pytest.raises(ValueError):
            m.remove_target_points(*w1, pose=p1)                     # a pose is applied on the device


def test_removing_points_that_are_not_in_the_map_is_an_error_3d(M, scans):
    from gtsam_ndt_amd import _lib as L
    (s0, p0), (s1, p1) = scans[0], scans[1]
    w0, w1 = _world(*s0, p0), _world(*s1, p1)

    def expect_mismatch(m, call):
        with pytest.raises(L.NdtError) as e:
            call()
        assert e.value.code == L.NDT_ERR_INVALID_ARG and "not in the target" in str(e.value)
        with pytest.raises(L.NdtError) as e:                         # no target afterwards, as after a failed add
            m.align(*s1, POSES[1])
        assert e.value.code == L.NDT_ERR_NO_TARGET
        m.reserve_target(LO, HI)                                     # ... and usable again
        assert m.add_target_points(*w0) >= 3
        assert m.align(*s1, POSES[1]).status == 0

    with M() as m:
        m.reserve_target(LO, HI)
        m.add_target_points(*w0)
        # a scan that was never added, over occupied voxels
        expect_mismatch(m, lambda: m.remove_target_points(*[_dev(c) for c in s1], pose=p1))
        # the same scan twice: the second time a count goes below zero
        m.add_target_points(*w1)
        m.remove_target_points(*w1)
        expect_mismatch(m, lambda: m.remove_target_points(*w1))
        # points shifted by 1 mm: a voxel of their own is emptied - its count reaches zero, its sums do not
        rng = np.random.default_rng(3)
        gi = m.grid_info()
        count = m.grid()[0].reshape(gi.depth, gi.height, gi.width)
        empty = np.argwhere(count[2:-2, 2:-2, 2:-2] == 0)
        iz, iy, ix = (int(v) + 2 for v in empty[len(empty) // 2])     # an empty voxel well inside the box
        q = [(np.float32(o) + np.float32(i) + rng.uniform(0.2, 0.8, 50).astype(np.float32)).astype(np.float32)
             for o, i in ((gi.ox, ix), (gi.oy, iy), (gi.oz, iz))]
        vox = [np.floor((c - np.float32(o)) * np.float32(gi.inv_cell)) for c, o in zip(q, (gi.ox, gi.oy, gi.oz))]
        assert [np.unique(v).tolist() for v in vox] == [[ix], [iy], [iz]]
        assert m.add_target_points(*q) == 0
        assert m.grid()[0].reshape(gi.depth, gi.height, gi.width)[iz, iy, ix] == 50
        expect_mismatch(m, lambda: m.remove_target_points(q[0] + np.float32(0.001), q[1], q[2]))


def test_scattered_fallback_3d(M, scans):
    """140 x 140 x 36 m at 1 m voxels: 36 x 36 x 10 tiles > 8192 - k_accumulate3 + k_finalise3."""
    from gtsam_ndt_amd import _lib as L
    (s0, p0) = scans[0]
    lo, hi = (-70.0, -70.0, -18.0), (70.0, 70.0, 18.0)
    d0 = [_dev(c) for c in s0]
    with M() as m, M() as fresh:
        gi = m.reserve_target(lo, hi)
        assert ((gi.width + 3) // 4) * ((gi.height + 3) // 4) * ((gi.depth + 3) // 4) > 8192
        fresh.reserve_target(lo, hi)
        out = m.add_target_points(*d0, pose=p0)
        assert m.grid_info().n_valid > 100 and m.grid()[0].sum() == s0[0].size - out
        assert m.remove_target_points(*d0, pose=p0) == out
        _assert_same_state(_state(m), _state(fresh))
        with pytest.raises(L.NdtError) as e:                         # and the mismatch rule holds on this path
            m.remove_target_points(*d0, pose=p0)
        assert e.value.code == L.NDT_ERR_INVALID_ARG
