"""Coarse-to-fine map-to-map alignment between STORED submaps (NdtMapPyramid2D / NdtMapPyramid3D): both submaps are built,
saved and closed; the pyramids come from the blobs alone, their coarse levels from ndt*_coarsen_map.

3D: the stock pair of tests/d2d3_ref.py at 1 m, which from the zero guess ends in a local optimum 0.25 m from the
generating pose (test_gpu_d2d3.py::test_coarse_then_fine_gets_past_the_local_optimum); one coarse level at 2 m with that
test's 2 m parameters.  Criterion of that test: NDT_OK, within 0.01 m / 1e-3 rad of the generating pose, while the fine pair
alone stays more than 0.1 m off.
2D: the config-2 scene at its size (50 m room, 100 000 points a side) started T_SURVEY = 0.30 m / -0.20 m / 0.05 rad from
the generating pose, default PYRAMID_LEVELS, and the tolerance NdtPyramid2D's own test holds that scene to
(test_gpu_survey_offsets.py: 5e-3 m, 5e-4 rad against the generating pose).  The reference is the same schedule with every
level built from the points, and it must meet that tolerance itself (asserted first).  It does with 1 cm of range noise
(measured on one MI355X: 0.44 mm / 0.33 mrad); at the workload's stock 3 cm, map-to-map alignment of two samplings of one
room ends 4.0 mm / 1.0 mrad off for 100 000, 200 000 and 400 000 points alike - the objective's own bias, from points as
from blobs - which the rotation tolerance does not admit, so the scans here carry sigma = 0.01.

The gap between the from-blob and the from-points final poses is printed and held to the file's POSE_TOL: the geometry is
the same and the sums differ by the roundings of section 2.17; measured 1.4e-8 m / 8e-10 rad (3D) and 6.1e-9 m / 8e-10 rad
(2D), four orders below the bound."""
import numpy as np
import pytest

from gtsam_ndt_amd import synth, synth3d

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-4
T_SURVEY = np.array([0.30, -0.20, 0.05])


def _from_points_schedule(Matcher, fine_params, levels, target, source, zero):
    """The same schedule with every level's pair of handles built from the points (what a caller who still has them does)."""
    from gtsam_ndt_amd.matcher import map_level_params
    from gtsam_ndt_amd import _lib as L
    fine_kw = {k: getattr(fine_params, k) for k, _ in L.Params2D._fields_ if not k.startswith("reserved")}
    pose, r = zero, None
    for kw in [map_level_params(fine_params, lv) for lv in levels] + [fine_kw]:
        with Matcher(**kw) as t, Matcher(**kw) as s:
            t.set_target(*target)
            s.set_target(*source)
            r = t.align_map(s, pose)
            assert r.status in (L.NDT_OK, L.NDT_NOT_CONVERGED)
            pose = r.pose
    return r


def test_stored_3d_submaps_get_past_the_local_optimum(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMapPyramid3D, NdtMatcher3D
    d = synth3d.make_pair3d()
    truth = np.array(d["pose"])
    zero = (0.0,) * 6
    levels = ((2.0, {}),)                                   # 2 m voxels, every other parameter as the 1 m handles'
    target, source = (d["tx"], d["ty"], d["tz"]), (d["sx"], d["sy"], d["sz"])
    with NdtMatcher3D(cell_size=1.0) as t1, NdtMatcher3D(cell_size=1.0) as s1:
        t1.set_target(*target)
        s1.set_target(*source)
        direct = t1.align_map(s1, zero)
        fine_params = t1.params
        blob_t, blob_s = t1.save_map(), s1.save_map()
    with NdtMapPyramid3D.from_blob(blob_t, levels=levels) as pt, NdtMapPyramid3D.from_blob(blob_s, levels=levels) as ps:
        assert [m.params.cell_size for m in pt.levels] == [2.0, 1.0]
        r = pt.align_map(ps, zero)
    ref = _from_points_schedule(NdtMatcher3D, fine_params, levels, target, source, zero)
    e, e_direct, e_ref = (np.abs(np.array(x.pose) - truth) for x in (r, direct, ref))
    gap = np.abs(np.array(r.pose) - np.array(ref.pose))
    print(f"3D from blobs: {r.iterations} iterations, {e[:3].max():.4f} m {e[3:].max():.5f} rad from the generating pose; from points "
          f"{e_ref[:3].max():.4f} m {e_ref[3:].max():.5f} rad; gap between the two {gap[:3].max():.3e} m {gap[3:].max():.3e} rad; "
          f"fine pair alone {e_direct[:3].max():.3f} m")
    assert r.status == 0
    assert e[:3].max() < 0.01 and e[3:].max() < 1e-3
    assert e_direct[:3].max() > 0.1
    assert gap.max() < POSE_TOL


def test_stored_2d_submaps_through_the_default_levels(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMapPyramid2D, NdtMatcher2D, PYRAMID_LEVELS
    d = synth.make_pair(2, sigma=0.01)
    xt, yt, xs, ys, pose = d["tx"], d["ty"], d["sx"], d["sy"], d["pose"]
    zero = tuple(np.array(pose) - T_SURVEY)                 # the start: the survey's offset from the generating pose
    with NdtMatcher2D() as t, NdtMatcher2D() as s:
        t.set_target(xt, yt)
        s.set_target(xs, ys)
        fine_params = t.params
        blob_t, blob_s = t.save_map(), s.save_map()
    ref = _from_points_schedule(NdtMatcher2D, fine_params, PYRAMID_LEVELS, (xt, yt), (xs, ys), zero)
    e_ref = np.abs(np.array(ref.pose) - np.array(pose))
    with NdtMapPyramid2D.from_blob(blob_t) as pt, NdtMapPyramid2D.from_blob(blob_s) as ps:
        assert [m.params.cell_size for m in pt.levels] == [2.0, 1.0, 0.5]
        r = pt.align_map(ps)
    e = np.abs(np.array(r.pose) - np.array(pose))
    gap = np.abs(np.array(r.pose) - np.array(ref.pose))
    print(f"2D from blobs: {r.iterations} iterations, {e.max():.2e} from the generating pose; from points {e_ref.max():.2e}; "
          f"gap between the two {gap[:2].max():.3e} m {gap[2]:.3e} rad")
    assert ref.status == 0 and e_ref[:2].max() < 5e-3 and e_ref[2] < 5e-4      # the inputs: the from-points schedule meets the tolerance
    assert r.status == 0 and e[:2].max() < 5e-3 and e[2] < 5e-4
    assert gap.max() < POSE_TOL
