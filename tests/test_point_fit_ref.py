"""CPU test of tests/point_fit_ref.py itself (no device): the classes partition the scan, selection is stable, and m
agrees with oracle.ndt2d.evaluate_one on single-point scans through score = d1 exp(-d2 / 2 m).  The grids are the
oracle's, from the committed fixtures."""
import math

import numpy as np
import pytest

import point_fit_cases as PC
import point_fit_ref as F
from oracle import ndt2d as o2
from oracle import ndt3d as o3


@pytest.fixture(scope="module")
def scene2():
    fx = PC.fixture(2)
    out = {}
    for ov in (1, 4):
        prm = o2.NdtParams(overlap=ov)
        grids = o2.build_grids(*fx["target"], prm)
        out[ov] = (prm, grids, F.records_of_oracle(grids))
    return fx, out


@pytest.fixture(scope="module")
def scene3():
    fx = PC.fixture(3)
    prm = o3.Ndt3Params()
    grid = o3.build_grid3(*fx["target"], prm)
    return fx, prm, grid, F.records_of_oracle(grid)


def test_fixture_counts_at_the_final_pose(scene2, scene3):
    """The figures the thresholds of the GPU tests were chosen by: no hit lies within its tolerance of max_m."""
    fx, by = scene2
    r = F.fit_ref(by[1][2], fx["source"], fx["final_pose"], PC.MAX_M[2])
    assert F.counts(r["cls"]) == dict(n_invalid=0, n_miss=162, n_misfit=189, n_fit=649)
    assert not (np.abs(r["m"][r["hit"]] - PC.MAX_M[2]) <= r["tol"][r["hit"]]).any()
    fx3, _, _, rec3 = scene3
    r = F.fit_ref(rec3, fx3["source"], fx3["final_pose"], PC.MAX_M[3])
    assert F.counts(r["cls"]) == dict(n_invalid=0, n_miss=2123, n_misfit=756, n_fit=1217)
    assert not (np.abs(r["m"][r["hit"]] - PC.MAX_M[3]) <= r["tol"][r["hit"]]).any()


@pytest.mark.parametrize("dim,ov", [(2, 1), (2, 4), (3, 1)])
def test_classes_partition_the_scan_and_selection_is_stable(scene2, scene3, dim, ov):
    if dim == 2:
        fx, by = scene2
        rec = by[ov][2]
    else:
        fx, _, _, rec = scene3
    cases = [(fx["source"], fx["final_pose"]), (fx["source"], PC.far_pose(dim, fx["final_pose"]))]
    if dim == 3:
        cases.append(PC.steep_scene(fx))
    for source, pose in cases:
        n = 2500
        coords, inj = PC.mixed_scan(rec, source, pose, n)
        r = F.fit_ref(rec, coords, pose, PC.MAX_M[dim])
        cls = r["cls"]
        c = F.counts(cls)
        assert sum(c.values()) == n and set(np.unique(cls)) <= {0, 1, 2, 3}
        assert np.all(cls[inj["bad"]] == F.INVALID) and c["n_invalid"] == len(inj["bad"])
        assert np.all(cls[inj["far"]] == F.MISS) and np.all(cls[inj["ring"]] == F.MISS)
        assert np.all((cls[inj["displaced"]] == F.MISS) | (cls[inj["displaced"]] == F.MISFIT))
        # m: a number for a hit, +inf for a miss, NaN for an invalid point
        assert np.all(np.isfinite(r["m"][cls >= F.MISFIT])) and np.all(np.isposinf(r["m"][cls == F.MISS]))
        assert np.all(np.isnan(r["m"][cls == F.INVALID]))
        assert np.all((cls == F.FIT) == (r["hit"] & r["finite"] & (r["m"].astype(np.float32) <= np.float32(PC.MAX_M[dim]))))
        total = 0
        for keep in range(1, 16):
            sel, idx = F.select_ref(coords, cls, keep)
            assert np.all(np.diff(idx) > 0)
            assert np.all(F.keep_mask(cls[idx], keep)) and not F.keep_mask(np.delete(cls, idx), keep).any()
            for a in range(dim):
                assert sel[a].tobytes() == coords[a][idx].tobytes()
            total += len(idx)
        assert total == 8 * n                              # every point is in 8 of the 15 masks
    if dim == 2 and ov == 1:
        assert c["n_fit"] > 0 and c["n_misfit"] > 0 and c["n_miss"] > 0


def test_displaced_outliers_do_not_fit(scene2, scene3):
    """0.25 m along the minor axis of the hit cell, 200 of them: what the GPU suite's map-update test relies on."""
    for dim, (fx, rec) in ((2, (scene2[0], scene2[1][1][2])), (3, (scene3[0], scene3[3]))):
        pose = fx["final_pose"]
        src, d = PC.displaced_outliers(rec, fx["source"], pose, 200)
        assert len(np.unique(src)) == 200
        rd = F.fit_ref(rec, tuple(d[:, a] for a in range(dim)), pose, PC.MAX_M[dim])
        assert np.all((rd["cls"] == F.MISS) | (rd["cls"] == F.MISFIT))
        moved = np.stack(fx["source"], axis=1)[src].astype(np.float64) - d.astype(np.float64)
        assert np.allclose(np.linalg.norm(moved, axis=1), 0.25, atol=1e-5)
        _, d = PC.displaced_outliers(rec, fx["source"], pose, 200, misfit_only=True)
        assert np.all(F.fit_ref(rec, tuple(d[:, a] for a in range(dim)), pose, PC.MAX_M[dim])["cls"] == F.MISFIT)


@pytest.mark.parametrize("ov", [1, 4])
def test_m_agrees_with_the_oracle_point_by_point_2d(scene2, ov):
    fx, by = scene2
    prm, grids, rec = by[ov]
    pose = fx["final_pose"]
    sx, sy = fx["source"]
    r = F.fit_ref(rec, (sx, sy), pose, PC.MAX_M[2])
    checked = 0
    for i in np.linspace(0, len(sx) - 1, 120).astype(np.int64):
        per_grid = [o2.evaluate_one(g, sx[i:i + 1], sy[i:i + 1], pose, prm, mirror32=True) for g in grids]
        hits = [(sc, nh) for _, _, sc, nh in per_grid if nh == 1]
        assert (len(hits) > 0) == bool(r["hit"][i])
        if hits:
            # score = d1 exp(-d2 / 2 m): the grid with the largest score has the least m
            m = -2.0 / prm.d2 * math.log(max(sc for sc, _ in hits) / prm.d1)
            assert abs(m - r["m"][i]) <= 1e-6 * max(1.0, abs(m)) + r["tol"][i]
            checked += 1
    assert checked > 60


def test_m_agrees_with_the_oracle_point_by_point_3d(scene3):
    fx, prm, grid, rec = scene3
    pose = fx["final_pose"]
    sx, sy, sz = fx["source"]
    r = F.fit_ref(rec, (sx, sy, sz), pose, PC.MAX_M[3])
    checked = 0
    for i in np.linspace(0, len(sx) - 1, 120).astype(np.int64):
        _, _, sc, nh = o3.evaluate3(grid, sx[i:i + 1], sy[i:i + 1], sz[i:i + 1], pose, prm, mirror32=True)
        assert (nh == 1) == bool(r["hit"][i])
        if nh == 1 and sc > 1e-300:
            m = -2.0 / prm.d2 * math.log(sc / prm.d1)
            assert abs(m - r["m"][i]) <= 1e-6 * max(1.0, abs(m)) + r["tol"][i]
            checked += 1
    assert checked > 30


def test_exact_pose_images_are_single_float32_adds():
    for dim in (2, 3):
        assert F.is_exact_pose(PC.EXACT_POSE[dim], dim)
        assert not F.is_exact_pose(PC.fixture(dim)["final_pose"], dim)
        R, t = F.rotation32(PC.EXACT_POSE[dim], dim)
        assert np.array_equal(R, np.eye(dim)) and np.array_equal(t, np.array(PC.EXACT_POSE[dim][:dim]))


def test_the_steep_scene_is_the_fixture_seen_from_a_tilted_frame(scene3):
    """steep_scene: the same images as the final pose's to float32 rounding of the source (3 half-ulps of 25 m), so the
    reference classes nearly every point as there - and the counts stay those of a mixed scene."""
    fx, _, _, rec = scene3
    source, pose = PC.steep_scene(fx)
    assert abs(pose[3]) >= 0.5 and abs(pose[4]) >= 0.5
    R0, t0 = F.rotation32(fx["final_pose"], 3)
    R1, t1 = F.rotation32(pose, 3)
    a = np.stack(fx["source"], 1).astype(np.float64) @ R0.T + t0
    b = np.stack(source, 1).astype(np.float64) @ R1.T + t1
    assert np.abs(a - b).max() < 6 * 2.0 ** -24 * np.abs(a).max()          # the source's rounding, and the two float32 R
    r0 = F.fit_ref(rec, fx["source"], fx["final_pose"], PC.MAX_M[3])
    r1 = F.fit_ref(rec, source, pose, PC.MAX_M[3])
    c = F.counts(r1["cls"])
    assert int((r0["cls"] != r1["cls"]).sum()) <= 8 and c["n_fit"] > 1000 and c["n_misfit"] > 500 and c["n_miss"] > 1500
