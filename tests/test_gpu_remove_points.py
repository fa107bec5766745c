"""ndt2d_remove_target_points(_dev): taking a scan out of a submap is the exact inverse of adding it.

Every expectation comes from the library's own build / add path (which other tests pin to the oracle) or from
oracle.ndt2d.build_grid on the points that should remain - never from the removal itself.  Each case runs under
binned_build = 0 (scattered atomics), 1 (chunk-sorted) and 2 (round-1 binned) against ONE expectation built with the default
path, so the three variants agree with it and with each other."""
import math

import numpy as np
import pytest

from gtsam_ndt_amd import synth
from handle_life import moved2d as _world      # ndt2d_add_target_points_dev's float32 restatement

pytestmark = pytest.mark.gpu

VARIANTS = (0, 1, 2)
POSES = [(8.0 + 1.5 * k, 10.0 + 0.8 * k, 0.1 * k) for k in range(6)]


def _state(m):
    """Everything the contract names: the sums (save_map), the records, the counts."""
    gi = m.grid_info()
    return {"map": m.save_map().tobytes(), "grid": m.grid(), "info": (gi.width, gi.height, gi.ox, gi.oy, gi.n_valid, gi.n_points)}


def _assert_same_state(got, want):
    assert got["info"] == want["info"]
    for u, v in zip(got["grid"], want["grid"]):
        np.testing.assert_array_equal(u, v)
    assert got["map"] == want["map"]


def _same_result(a, b):
    return a.pose == b.pose and a.iterations == b.iterations and a.score == b.score and a.status == b.status and a.n_hit == b.n_hit


@pytest.fixture(scope="module")
def M(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    return NdtMatcher2D


@pytest.fixture(scope="module")
def room(gpu_lib):
    """Four 7 200-beam scans of a 30 m room, NaN beams included, the poses an alignment would have returned, and the map
    points T (scan 0 in the world frame) with the extreme points of everything the tests put into the map."""
    sc = synth.room_scene(4242, 30.0)
    scans = {}
    for name, k, dp in (("T", 0, (0.0, 0.0, 0.0)), ("A", 2, (0.003, -0.002, 0.0004)), ("B", 4, (-0.002, 0.004, -0.0003)),
                        ("C", 3, (0.0, 0.0, 0.0))):
        r, a0, da = synth.lidar_scan2d(sc, POSES[k], n_beams=7200, seed=100 + k)
        x, y = synth.scan_points(r, a0, da)
        x[[17, 4000, 7199]] = np.nan; y[[17, 4000, 7199]] = np.nan            # no-return beams, whatever the scene gives
        pose = tuple(np.array(POSES[k]) + np.array(dp))
        scans[name] = (x, y, pose)
    x0, y0, p0 = scans["T"]
    ok = ~np.isnan(x0)
    tx, ty = _world(x0[ok], y0[ok], p0)
    pose_a2 = (scans["A"][2][0] + 0.21, scans["A"][2][1] - 0.13, scans["A"][2][2] + 0.02)      # A re-anchored after a loop closure
    ex, ey = [tx], [ty]
    for name, pose in (("A", scans["A"][2]), ("A", pose_a2), ("B", scans["B"][2])):
        wx, wy = _world(scans[name][0], scans[name][1], pose)
        ex.append(wx[~np.isnan(wx)]); ey.append(wy[~np.isnan(wy)])
    ex, ey = np.concatenate(ex), np.concatenate(ey)
    # two corner points carry the extent: every grid below has the geometry of the rebuild it is compared with
    tx = np.concatenate([tx, np.float32([ex.min() - 1.0, ex.max() + 1.0])])
    ty = np.concatenate([ty, np.float32([ey.min() - 1.0, ey.max() + 1.0])])
    return {"tx": tx, "ty": ty, "scans": scans, "pose_a2": pose_a2}


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _valid_world(scan, pose):
    wx, wy = _world(scan[0], scan[1], pose)
    ok = ~np.isnan(wx)
    return wx[ok], wy[ok]


@pytest.fixture(scope="module")
def inverse_expected(M, room):
    """set_target(T); add(B, pb) - on the default build path - and an alignment of scan C against it."""
    B, Cs = room["scans"]["B"], room["scans"]["C"]
    with M() as m:
        m.set_target(room["tx"], room["ty"])
        out_b = m.add_target_points(_dev(B[0]), _dev(B[1]), pose=B[2])
        st = _state(m)
        guess = (Cs[2][0] + 0.05, Cs[2][1] - 0.04, Cs[2][2] + 0.01)
        r = m.align(_dev(Cs[0]), _dev(Cs[1]), guess)
    assert r.status == 0
    return {"state": st, "out_b": out_b, "align": r, "guess": guess}


@pytest.mark.parametrize("variant", VARIANTS)
def test_remove_is_the_exact_inverse_of_add(M, room, inverse_expected, variant):
    """7 200 points per scan: split_points is 1 024, so the one to four tiles of the room are shared by several workgroups
    and the list hand-off of the sorted build carries negative partial counts."""
    from oracle import ndt2d as o
    A, B, Cs = room["scans"]["A"], room["scans"]["B"], room["scans"]["C"]
    exp = inverse_expected
    with M(tuning={"binned_build": variant}) as m:
        m.set_target(room["tx"], room["ty"])
        ax, ay, bx, by = _dev(A[0]), _dev(A[1]), _dev(B[0]), _dev(B[1])
        out_a = m.add_target_points(ax, ay, pose=A[2])
        out_b = m.add_target_points(bx, by, pose=B[2])
        n_with_a = m.grid_info().n_points
        out_r = m.remove_target_points(ax, ay, pose=A[2])
        assert out_r == out_a >= 3 and out_b == exp["out_b"]                 # (the NaN beams count as outside, both ways)
        st = _state(m)
        _assert_same_state(st, exp["state"])
        assert n_with_a - st["info"][5] == A[0].size - out_a > 6000           # the scan did go in and out
        r = m.align(_dev(Cs[0]), _dev(Cs[1]), exp["guess"])
        assert _same_result(r, exp["align"]), (r, exp["align"])
    wbx, wby = _valid_world(B, B[2])
    g = o.build_grid(np.concatenate([room["tx"], wbx]), np.concatenate([room["ty"], wby]), o.NdtParams())
    np.testing.assert_array_equal(st["grid"][0].astype(np.int64), g.count)
    assert st["info"][:2] == (g.W, g.H) and st["info"][4] == g.n_valid


@pytest.mark.parametrize("variant", VARIANTS)
def test_interleaved_adds_and_removes_equal_rebuilds(M, room, variant):
    """add A, add B, remove A, add A at another pose, remove B: after each step the grid is the one a build from what
    should remain gives (set_target on the float32-transformed points, default path)."""
    A, B = room["scans"]["A"], room["scans"]["B"]
    pa, pa2, pb = A[2], room["pose_a2"], B[2]
    ax, ay, bx, by = _dev(A[0]), _dev(A[1]), _dev(B[0]), _dev(B[1])
    dev = {"A": (ax, ay), "B": (bx, by)}
    steps = [("add", "A", pa, [("A", pa)]), ("add", "B", pb, [("A", pa), ("B", pb)]),
             ("remove", "A", pa, [("B", pb)]), ("add", "A", pa2, [("B", pb), ("A", pa2)]),
             ("remove", "B", pb, [("A", pa2)])]
    with M(tuning={"binned_build": variant}) as m, M() as ref:
        m.set_target(room["tx"], room["ty"])
        for op, scan, pose, remain in steps:
            out = (m.add_target_points if op == "add" else m.remove_target_points)(*dev[scan], pose=pose)
            assert out == int(np.isnan(room["scans"][scan][0]).sum()) >= 3      # the NaN beams, nothing else
            parts = [(room["tx"], room["ty"])] + [_valid_world(room["scans"][name], p) for name, p in remain]
            ref.set_target(np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
            _assert_same_state(_state(m), _state(ref))


@pytest.fixture(scope="module")
def pair2(gpu_lib):
    d = synth.make_pair(2, n_tgt=60000, n_src=20000)               # a 50 m room: 4 x 4 tiles, the last row partial
    with_default = {}
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    with NdtMatcher2D() as m:
        m.set_target(d["tx"], d["ty"])
        with_default["state"] = _state(m)
        with_default["align"] = m.align(d["sx"], d["sy"], d["init"])
    return d, with_default


@pytest.mark.parametrize("variant", VARIANTS)
def test_other_tile_situations(M, pair2, variant):
    """The host entry point (no pose); a removal that touches one tile of sixteen; one lying wholly outside; a cloud smaller
    than a wave.  After each add + remove the grid is the one set_target alone gives."""
    d, exp = pair2
    tx, ty = d["tx"], d["ty"]
    corner = (tx < tx.min() + 6) & (ty < ty.min() + 6)
    assert 100 < corner.sum() < tx.size // 8
    with M(tuning={"binned_build": variant}) as m:
        m.set_target(tx, ty)
        # one tile touched, fifteen leave at once
        assert m.add_target_points(tx[corner], ty[corner]) == 0
        assert m.grid_info().n_points == tx.size + corner.sum()
        assert m.remove_target_points(tx[corner], ty[corner]) == 0
        _assert_same_state(_state(m), exp["state"])
        # every tile shared: a third of the cloud, through the host entry point
        assert m.add_target_points(tx[::3], ty[::3]) == 0
        assert m.remove_target_points(tx[::3], ty[::3]) == 0
        _assert_same_state(_state(m), exp["state"])
        # wholly outside: counted, nothing changes
        assert m.remove_target_points(tx[:50] + np.float32(500.0), ty[:50]) == 50
        _assert_same_state(_state(m), exp["state"])
        # fewer points than a wave, on the device, moved by a pose
        sx, sy = _dev(d["sx"][:40]), _dev(d["sy"][:40])
        out = m.add_target_points(sx, sy, pose=d["pose"])
        assert m.grid_info().n_points == tx.size + 40 - out
        assert m.remove_target_points(sx, sy, pose=d["pose"]) == out
        _assert_same_state(_state(m), exp["state"])
        r = m.align(d["sx"], d["sy"], d["init"])
        assert _same_result(r, exp["align"])
        with pytest.raises(ValueError):
            m.remove_target_points(tx[:10], ty[:10], pose=(0.0, 0.0, 0.0))   # a pose is applied on the device


@pytest.mark.parametrize("variant", VARIANTS)
def test_remove_everything_equals_a_fresh_reserve(M, pair2, variant):
    from gtsam_ndt_amd import _lib as L
    d, _ = pair2
    tx, ty = d["tx"], d["ty"]
    box = (tx.min(), ty.min(), tx.max(), ty.max())
    with M(tuning={"binned_build": variant}) as m, M() as fresh:
        m.reserve_target(*box)
        fresh.reserve_target(*box)
        assert m.add_target_points(tx, ty) == 0
        assert m.grid_info().n_valid > 100
        assert m.remove_target_points(tx, ty) == 0
        gi = m.grid_info()
        assert gi.n_valid == 0 and gi.n_points == 0
        _assert_same_state(_state(m), _state(fresh))
        r = m.align(d["sx"], d["sy"], d["init"])
        assert r.status == L.NDT_TOO_FEW_CELLS and r.iterations == 0


@pytest.mark.parametrize("variant", VARIANTS)
def test_a_cell_that_drops_below_min_points_becomes_invalid(M, variant):
    rng = np.random.default_rng(5)
    # a wall of well-filled cells, and one cell [5.0, 5.5) x [7.0, 7.5) that holds exactly min_points = 3 points
    wx = rng.uniform(1.0, 9.0, 400).astype(np.float32)
    wy = (2.0 + rng.normal(0, 0.02, 400)).astype(np.float32)
    px = np.float32([5.1, 5.3, 5.4]); py = np.float32([7.1, 7.4, 7.2])
    with M(tuning={"binned_build": variant}) as m:
        gi = m.reserve_target(0.0, 0.0, 10.0, 10.0)
        m.add_target_points(np.concatenate([wx, px]), np.concatenate([wy, py]))
        before = _state(m)
        cell = int(math.floor((7.1 - gi.oy) * gi.inv_cell)) * gi.width + int(math.floor((5.1 - gi.ox) * gi.inv_cell))
        count, mean, icov = before["grid"]
        assert count[cell] == 3 and icov[cell].any()
        assert m.remove_target_points(px[:1], py[:1]) == 0
        count, mean, icov = m.grid()
        assert count[cell] == 2 and not mean[cell].any() and not icov[cell].any()          # two points left, the record is zero
        info = m.grid_info()
        assert info.n_valid == before["info"][4] - 1 and info.n_points == before["info"][5] - 1
        others = np.arange(count.size) != cell
        for u, v in zip((count, mean, icov), before["grid"]):
            np.testing.assert_array_equal(u[others], v[others])
        assert m.add_target_points(px[:1], py[:1]) == 0
        _assert_same_state(_state(m), before)


def test_overlapping_grids_leave_all_four(M, pair2):
    d, _ = pair2
    tx, ty = d["tx"], d["ty"]
    half = len(tx) // 2
    ext = np.unique([np.argmin(tx), np.argmax(tx), np.argmin(ty), np.argmax(ty)])
    first = np.union1d(np.arange(half), ext)
    rest = np.setdiff1d(np.arange(len(tx)), first)
    out = {}
    for variant in ("expected",) + VARIANTS:
        kw = {} if variant == "expected" else {"tuning": {"binned_build": variant}}
        with M(overlap_grids=4, **kw) as m:
            m.set_target(tx[first], ty[first])
            m.add_target_points(tx[rest], ty[rest])
            if variant != "expected":
                extra = rest[::2]
                assert m.add_target_points(tx[extra], ty[extra]) == 0
                assert m.grid_info().n_points == tx.size + extra.size
                assert m.remove_target_points(tx[extra], ty[extra]) == 0
            r = m.align(d["sx"], d["sy"], d["init"])
            gi = m.grid_info()
            out[variant] = (gi.n_valid, gi.n_points, r.pose, r.iterations, r.score, m.save_map().tobytes())
    for variant in VARIANTS:
        assert out[variant] == out["expected"], variant


def test_scattered_fallback(M):
    """1.6 km x 1.6 km at 0.5 m: 100 x 100 tiles > 8192, scattered atomics and k_finalise whatever the knob says."""
    from gtsam_ndt_amd import _lib as L
    rng = np.random.default_rng(11)
    n = 20_000
    x = rng.uniform(0, 1600, n).astype(np.float32)
    y = (800 + 700 * np.sin(x / 120.0) + rng.normal(0, 0.05, n)).astype(np.float32)
    sx = rng.uniform(300, 340, 4000).astype(np.float32)
    sy = (800 + 700 * np.sin(sx / 120.0) + rng.normal(0, 0.05, 4000)).astype(np.float32)
    with M() as m:
        info = m.set_target(x, y)
        assert ((info.width + 31) // 32) * ((info.height + 31) // 32) > 8192
        before = (m.grid(), info.n_valid, m.grid_info().n_points)
        assert m.add_target_points(sx, sy) == 0
        mid = m.grid_info()
        assert mid.n_points == n + 4000 and mid.n_valid > info.n_valid
        assert m.remove_target_points(_dev(sx), _dev(sy), pose=(0.0, 0.0, 0.0)) == 0
        after = (m.grid(), m.grid_info().n_valid, m.grid_info().n_points)
        assert after[1:] == before[1:]
        for u, v in zip(after[0], before[0]):
            np.testing.assert_array_equal(u, v)
        with pytest.raises(L.NdtError) as e:                                   # and the mismatch rule holds on this path
            m.remove_target_points(sx, sy)
        assert e.value.code == L.NDT_ERR_INVALID_ARG


@pytest.mark.parametrize("variant", VARIANTS)
def test_removing_points_that_are_not_in_the_map_is_an_error(M, room, variant):
    from gtsam_ndt_amd import _lib as L
    A, Cs = room["scans"]["A"], room["scans"]["C"]
    wax, way = _valid_world(A, A[2])
    guess = (Cs[2][0] + 0.05, Cs[2][1] - 0.04, Cs[2][2] + 0.01)

    def expect_mismatch(m, call):
        with pytest.raises(L.NdtError) as e:
            call()
        assert e.value.code == L.NDT_ERR_INVALID_ARG and "not in the target" in str(e.value)
        with pytest.raises(L.NdtError) as e:                                   # no target afterwards, as after a failed add
            m.align(Cs[0], Cs[1], guess)
        assert e.value.code == L.NDT_ERR_NO_TARGET
        m.set_target(room["tx"], room["ty"])                                   # ... and usable again
        assert m.align(Cs[0], Cs[1], guess).status == 0

    with M(tuning={"binned_build": variant}) as m:
        m.set_target(room["tx"], room["ty"])
        # a scan that was never added, over occupied cells
        expect_mismatch(m, lambda: m.remove_target_points(_dev(A[0]), _dev(A[1]), pose=A[2]))
        # the same scan twice: the second time a count goes below zero
        m.add_target_points(wax, way)
        assert m.remove_target_points(wax, way) == 0
        expect_mismatch(m, lambda: m.remove_target_points(wax, way))
        # points shifted by 1 mm: a cell of their own ([40.0, 40.5) x [3.0, 3.5) holds nothing else) is emptied - its count
        # reaches zero, its sums do not (1 mm = 8 389 units of cell_size / 2^22)
        rng = np.random.default_rng(variant)
        qx = np.float32(40.0) + rng.uniform(0.1, 0.4, 50).astype(np.float32)
        qy = np.float32(3.0) + rng.uniform(0.1, 0.4, 50).astype(np.float32)
        gi = m.reserve_target(0.0, 0.0, 50.0, 10.0)
        key = lambda px, py: (np.floor((py - gi.oy) * gi.inv_cell) * gi.width + np.floor((px - gi.ox) * gi.inv_cell)).astype(np.int64)
        assert np.unique(key(qx, qy)).size == 1 and np.array_equal(key(qx + np.float32(0.001), qy), key(qx, qy))
        assert m.add_target_points(qx, qy) == 0
        expect_mismatch(m, lambda: m.remove_target_points(qx + np.float32(0.001), qy))


@pytest.mark.parametrize("variant", VARIANTS)
def test_removal_invalidates_what_map_to_map_alignment_cached(M, room, variant):
    """align_map against a handle, remove a scan from it, align_map again: the second result is the one a handle built
    without that scan gives - the removal reached the D2D component lists and covariance records."""
    A, Cs = room["scans"]["A"], room["scans"]["C"]
    cx, cy = _valid_world(Cs, Cs[2])
    init = (0.05, -0.04, 0.01)
    with M(tuning={"binned_build": variant}) as m, M() as without, M() as other:
        other.set_target(cx, cy)
        without.set_target(room["tx"], room["ty"])
        m.set_target(room["tx"], room["ty"])
        m.add_target_points(_dev(A[0]), _dev(A[1]), pose=A[2])
        first_t, first_s = m.align_map(other, init), other.align_map(m, init)       # m as the target, m as the source
        m.remove_target_points(_dev(A[0]), _dev(A[1]), pose=A[2])
        second_t, second_s = m.align_map(other, init), other.align_map(m, init)
        want_t, want_s = without.align_map(other, init), other.align_map(without, init)
        assert _same_result(second_t, want_t), (second_t, want_t)
        assert _same_result(second_s, want_s), (second_s, want_s)
        assert not _same_result(first_t, second_t) and not _same_result(first_s, second_s)
        for u, v in zip(m.components(), without.components()):
            np.testing.assert_array_equal(u, v)
