"""ndt3d_set_map_neighbourhood(target, 7): in 3D map-to-map alignment a source component is scored against the target
voxel its mean falls into and that voxel's six face neighbours (docs/ALGORITHM.md section 2.26), against the float64
restatement tests/d2d3_nb_ref.py.

Bounds.  Evaluations: d2d3_nb_ref.eval_bounds_nb, the recipe of tests/test_gpu_d2d3.py - 4 x the restatement's own
largest float32-vs-float64 difference over the test's cases, floored at the project's 2e-5; H entries relative to
sqrt(H_aa H_bb), g to sqrt(H_aa score), H_aa of the Gauss-Newton form.  Poses: the project's 1e-4 m / 1e-4 rad against
the restatement, on cases whose float32 and float64 restatements agree within a quarter of that
(tests/test_d2d3_nb_ref.py: 9e-8 m on the stock pair).  Everything else is bitwise.

Scenes.  "small" = make_pair3d(6, 256) at 1 m voxels: 66 source components against 71 target voxels, one workgroup; no
component's image lies within 4 float32 ulps of a voxel face at `init` or at the generating pose (asserted), so n_hit
is compared exactly.  "near1m" and the stock pair are those of tests/test_gpu_d2d3.py.  The edge grid is
d2d3_nb_ref's: 6 x 5 x 4 voxels with six occupied voxels on its faces.

3D handles have no NDT_TUNE_LAUNCH_GRAPHS (ndt3d_set_tuning refuses the knob: a 3D chain always runs on graphs), so the
multi = single test varies what a 3D handle has: the mode of the loop and NDT_TUNE_MAP_MULTI_FROM; that the knob is
refused is asserted there."""
import numpy as np
import pytest

import d2d3_nb_ref as NB
import d2d3_ref as R
from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import synth3d
from oracle import ndt3d as O

pytestmark = pytest.mark.gpu

POSE_A = (0.10, -0.08, 0.02, 0.004, -0.003, 0.01)
POSE_TOL = 1e-4
ZERO = (0.0,) * 6
_cache = {}


def _pair(name):
    if name not in _cache:
        _cache[name] = {"small": lambda: synth3d.make_pair3d(n_elev=6, n_azim=256),
                        "near1m": lambda: synth3d.make_pair3d(pose=POSE_A, n_elev=32, n_azim=1024),
                        "stock": lambda: synth3d.make_pair3d()}[name]()
    return _cache[name]


def _ref_maps(name):
    """(target grid, source components, target's own components) of the restatement at 1 m voxels, once per scene"""
    if ("ref", name) not in _cache:
        d, prm = _pair(name), O.Ndt3Params(cell_size=1.0)
        tgt, own = R.build_map(d["tx"], d["ty"], d["tz"], prm)
        _, comps = R.build_map(d["sx"], d["sy"], d["sz"], prm)
        _cache[("ref", name)] = (tgt, comps, own)
    return _cache[("ref", name)]


def _ref_align(name, nb):
    if ("align", name, nb) not in _cache:
        tgt, comps, _ = _ref_maps(name)
        _cache[("align", name, nb)] = NB.align_nb(tgt, comps, ZERO, O.Ndt3Params(cell_size=1.0), nb)
    return _cache[("align", name, nb)]


def _matcher(x, y, z, **kw):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    kw.setdefault("cell_size", 1.0)
    m = NdtMatcher3D(**kw)
    m.set_target(x, y, z)
    return m


def _handles(name, **kw):
    d = _pair(name)
    skw = {k: v for k, v in kw.items() if k != "map_neighbourhood"}          # the setting is the target's
    return _matcher(d["tx"], d["ty"], d["tz"], **kw), _matcher(d["sx"], d["sy"], d["sz"], **skw)


def _same(a, b):
    return (a.pose == b.pose and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g) and a.score == b.score and
            a.iterations == b.iterations and a.n_hit == b.n_hit and a.status == b.status)


def _same_eval(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


# ------------------------------------------------------------------------------------------ 1. against the restatement
@pytest.mark.parametrize("mode", [0, 1])
def test_evaluate_map_matches_the_restatement(gpu_lib, mode):
    d = _pair("small")
    tgt, comps, _ = _ref_maps("small")
    prm, gn = O.Ndt3Params(cell_size=1.0, hessian_mode=mode), O.Ndt3Params(cell_size=1.0)
    poses = (d["init"], d["pose"])
    assert (comps.n, tgt.n_valid) == (66, 71)
    for pose in poses:
        assert NB.n_border(tgt, comps, pose) == 0                 # no failure below can hide behind a flipped voxel
    bound, worst = NB.eval_bounds_nb([(tgt, comps, p) for p in poses], prm)
    print(f"small, mode {mode}: float32 vs float64 of the restatement at 7 (H, g, score): {worst}; bound {bound}")
    t, s = _handles("small", hessian_mode=mode, map_neighbourhood=7)
    with t, s:
        assert t.map_neighbourhood == 7 and s.map_neighbourhood == 1
        for pose in poses:
            ref = NB.evaluate_nb(tgt, comps, pose, prm, 7)
            Hgn = NB.evaluate_nb(tgt, comps, pose, gn, 7)[0]
            got = t.evaluate_map(s, pose)
            diffs = R.eval_diffs(got, ref, Hgn)
            print(f"small, mode {mode}, pose {np.round(pose, 4)}: n_hit {got[3]} / {ref[3]}, (H, g, score) differences {diffs}")
            assert got[3] == ref[3], (got[3], ref[3])
            assert diffs[0] <= bound[0] and diffs[1] <= bound[1] and diffs[2] <= bound[2], (diffs, bound)
        t.set_map_neighbourhood(1)
        n1, n7 = t.evaluate_map(s, d["init"])[3], NB.evaluate_nb(tgt, comps, d["init"], prm, 7)[3]
        assert (n1, n7) == (60, 196)


# ----------------------------------------------------------------------------------------------- 2. edges, by index
def _edge_matcher(voxels, seed, **kw):
    """A matcher over the edge grid (reserved: a reserved 3D grid bins its ring voxels) with voxel_points in `voxels`"""
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    m = NdtMatcher3D(cell_size=1.0, **kw)
    info = m.reserve_target((1.0, 1.0, 1.0), (4.5, 3.5, 2.5))
    assert (info.ox, info.oy, info.oz) == (0.0, 0.0, 0.0) and (info.width, info.height, info.depth) == NB.EDGE_DIMS
    pts = np.concatenate([NB.voxel_points(v, seed) for v in voxels])
    assert m.add_target_points(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()) == 0
    assert m.grid_info().n_valid == len(voxels)
    return m, pts


def test_candidates_are_skipped_by_index(gpu_lib):
    """One component on each of six occupied face voxels whose keys are 1, W and 15 W apart: one pair each, where a
    neighbour by key arithmetic would make two; one voxel outside the grid: nothing."""
    prm = O.Ndt3Params(cell_size=1.0)
    t, pts = _edge_matcher(NB.EDGE_VOXELS, 5, map_neighbourhood=7)
    tgt, _ = NB.build_map_at(np.zeros(3), NB.EDGE_DIMS, pts[:, 0], pts[:, 1], pts[:, 2], prm)
    with t:
        for v in NB.EDGE_VOXELS:
            s, p = _edge_matcher([v], 9)
            _, comps = NB.build_map_at(np.zeros(3), NB.EDGE_DIMS, p[:, 0], p[:, 1], p[:, 2], prm)
            bound = NB.eval_bounds_nb([(tgt, comps, ZERO)], prm)[0]
            with s:
                assert s.components()[0].size == comps.n == 1
                ref = NB.evaluate_nb(tgt, comps, ZERO, prm, 7)
                got = t.evaluate_map(s, ZERO)
                print(f"voxel {v}: n_hit {got[3]} / {ref[3]}, score {got[2]} / {ref[2]}")
                assert got[3] == ref[3] == 1, v
                assert abs(got[2] - ref[2]) <= bound[2] * ref[2], (v, got[2], ref[2])
                for a in range(3):
                    for sgn, at_face in ((-1.0, v[a] == 0), (1.0, v[a] == NB.EDGE_DIMS[a] - 1)):
                        if at_face:                               # one voxel outside, next to the occupied voxel
                            pose = [0.0] * 6
                            pose[a] = sgn
                            H, g, sc, nh = t.evaluate_map(s, pose)
                            assert (sc, nh) == (0.0, 0) and not H.any() and not g.any(), (v, a, sgn)
        # a real face neighbour does count: the component of (4, 1, 1) has an empty own voxel and (5, 1, 1) at +x
        s, p = _edge_matcher([(4, 1, 1)], 9)
        _, comps = NB.build_map_at(np.zeros(3), NB.EDGE_DIMS, p[:, 0], p[:, 1], p[:, 2], prm)
        with s:
            ref, got = NB.evaluate_nb(tgt, comps, ZERO, prm, 7), t.evaluate_map(s, ZERO)
            assert got[3] == ref[3] == 1 and abs(got[2] - ref[2]) <= 2e-5 * ref[2]
            t.set_map_neighbourhood(1)
            assert t.evaluate_map(s, ZERO)[2:] == (0.0, 0)


# ----------------------------------------------------------------------------------------------- 3. converged alignment
def test_the_near_pair_converges_as_the_restatement_does(gpu_lib):
    ref = _ref_align("near1m", 7)
    t, s = _handles("near1m", map_neighbourhood=7)
    with t, s:
        r = t.align_map(s, ZERO)
    e = NB.pose_error(r.pose, ref["pose"])
    print(f"near1m at 7: {r.iterations} iterations (restatement {ref['iterations']}), status {r.status}, "
          f"{e[0]:.2e} m / {e[1]:.2e} rad from the restatement, n_hit {r.n_hit} / {ref['n_hit']}")
    assert r.status == ref["status"] == L.NDT_OK
    assert r.iterations == ref["iterations"] == 18
    assert e[0] < POSE_TOL and e[1] < POSE_TOL


def test_the_stock_pair_from_the_zero_guess_is_recovered_with_7(gpu_lib):
    """With the own voxel alone the stock pair ends in the local optimum DESIGN section 5.9 documents; with the face
    neighbours it ends where the restatement does, 1.6 mm / 0.24 mrad from the generating pose."""
    d = _pair("stock")
    ref = _ref_align("stock", 7)
    t, s = _handles("stock")
    with t, s:
        r1 = t.align_map(s, ZERO)
        t.set_map_neighbourhood(7)
        r7 = t.align_map(s, ZERO)
    e1, e7, et = NB.pose_error(r1.pose, d["pose"]), NB.pose_error(r7.pose, ref["pose"]), NB.pose_error(r7.pose, d["pose"])
    print(f"stock pair: with 1 {r1.iterations} iterations, {e1[0]:.4f} m / {e1[1]:.4f} rad from the generating pose; with 7 "
          f"{r7.iterations} iterations (restatement {ref['iterations']}), {e7[0]:.2e} m / {e7[1]:.2e} rad from the restatement, "
          f"{et[0]:.5f} m / {et[1]:.5f} rad from the generating pose, n_hit {r7.n_hit} / {ref['n_hit']}")
    assert r1.status == r7.status == L.NDT_OK
    assert e1[0] > 0.2
    assert e7[0] < POSE_TOL and e7[1] < POSE_TOL
    assert et[0] < 1e-2 and et[1] < 1e-3
    assert r7.iterations == ref["iterations"]


# ----------------------------------------------------------------------------------------------- 4. multi = single
@pytest.mark.parametrize("multi_from", [2, 65])
@pytest.mark.parametrize("fixed", [6, 0])
def test_every_start_of_a_multi_call_equals_its_single_alignment(gpu_lib, fixed, multi_from):
    d = _pair("small")
    t, s = _handles("small", fixed_iterations=fixed, map_neighbourhood=7)
    s2 = _matcher(d["sx"][::2], d["sy"][::2], d["sz"][::2])
    with t, s, s2:
        with pytest.raises(L.NdtError):                           # (a 3D chain always runs on graphs: nothing to vary)
            t.set_tuning("launch_graphs", 0)
        t.set_tuning("map_multi_from", multi_from)
        init = np.array(d["init"])
        poses = [ZERO, tuple(init), tuple(init + np.array([0.05, -0.04, 0.02, 0.004, -0.003, 0.01])), tuple(init), ZERO]
        sources = [s, s, s, s2, t]
        multi = t.align_map_multi(sources, poses)
        assert len(multi) == 5
        single = [t.align_map(src, p) for src, p in zip(sources, poses)]
        for k in range(5):
            assert _same(multi[k], single[k]), (k, multi[k], single[k])
        assert all(r.n_hit > 0 for r in single) and len({r.pose for r in single}) >= 4
        # ... and they are the neighbourhood's results, not the single-voxel ones
        t.set_map_neighbourhood(1)
        assert all(a.n_hit > b.n_hit for a, b in zip(single, [t.align_map(src, p) for src, p in zip(sources, poses)]))


# ----------------------------------------------------------------------------------------------- 5. switching
def test_switching_on_one_handle(gpu_lib):
    """A graph cached under one setting must not be replayed under the other: the single chain's and the multi chain's."""
    d = _pair("small")
    poses = [ZERO, d["init"], d["pose"]]
    t, s = _handles("small")
    f1, _ = _handles("small")
    f7, _ = _handles("small", map_neighbourhood=7)

    def run(m):
        m.set_tuning("map_multi_from", 2)
        return m.align_map(s, d["init"]), m.evaluate_map(s, d["init"]), m.align_map_multi(s, poses)

    def equal(a, b):
        return _same(a[0], b[0]) and _same_eval(a[1], b[1]) and all(_same(x, y) for x, y in zip(a[2], b[2]))

    with t, s, f1, f7:
        want = {1: run(f1), 7: run(f7)}
        assert not equal(want[1], want[7]) and want[7][1][3] > 2 * want[1][1][3]
        for nb in (1, 7, 1, 7):
            t.set_map_neighbourhood(nb)
            assert t.map_neighbourhood == nb
            assert equal(run(t), want[nb]), nb
        # the target's setting alone counts; the point neighbourhood is another setting
        s.set_map_neighbourhood(7)
        assert equal(run(t), want[7])
        t.set_map_neighbourhood(1)
        assert equal(run(t), want[1])
        s.set_map_neighbourhood(1)
        t.set_neighbourhood(7)
        assert t.map_neighbourhood == 1 and equal(run(t), want[1])
        t.set_map_neighbourhood(7)
        assert t.neighbourhood == 7 and equal(run(t), want[7])
        t.set_neighbourhood(1)
        assert equal(run(t), want[7])
        with pytest.raises(L.NdtError) as err:
            t.set_map_neighbourhood(3)
        assert err.value.code == L.NDT_ERR_INVALID_ARG and "ndt3d_set_map_neighbourhood" in str(err.value)
        assert t.map_neighbourhood == 7


# ----------------------------------------------------------------------------------------------- 6. a map against itself
@pytest.mark.parametrize("mode", [0, 1])
def test_a_map_against_itself_is_stationary_up_to_rounding(gpu_lib, mode):
    """Neighbour pairs (i -> j) and (j -> i) cancel in exact arithmetic, not in float32: g is small against its scale,
    not zero."""
    d = _pair("small")
    tgt, _, own = _ref_maps("small")
    prm, gn = O.Ndt3Params(cell_size=1.0, hessian_mode=mode), O.Ndt3Params(cell_size=1.0)
    assert NB.n_border(tgt, own, ZERO) == 0
    bound = NB.eval_bounds_nb([(tgt, own, ZERO)], prm)[0]
    ref = NB.evaluate_nb(tgt, own, ZERO, prm, 7)
    Hgn = NB.evaluate_nb(tgt, own, ZERO, gn, 7)[0]
    with _matcher(d["tx"], d["ty"], d["tz"], hessian_mode=mode, map_neighbourhood=7) as m:
        H, g, sc, nh = m.evaluate_map(m, ZERO)
    scale = np.sqrt(np.diag(Hgn) * sc)
    print(f"self, mode {mode}: n_hit {nh} / {ref[3]} of {own.n} components, score {sc}, |g| / sqrt(H_aa score) {np.abs(g) / scale}, "
          f"restatement float64 max|g| {np.abs(ref[1]).max():.2e}")
    assert nh == ref[3] > own.n
    assert np.all(np.abs(g) < bound[1] * scale), (np.abs(g) / scale, bound[1])
    assert abs(sc - ref[2]) <= bound[2] * ref[2]


# ----------------------------------------------------------------------------------------------- 7. refusals, persistence
def test_searches_and_pose_lists_refuse_while_the_target_is_at_7(gpu_lib):
    d = _pair("small")
    window = (d["pose"], (0.5, 0.5, 0.1), (0.25, 0.25, 0.05))
    rng = np.random.default_rng(11)
    poses = np.array(d["pose"]) + rng.uniform(-1, 1, (6, 6)) * np.array([0.3, 0.3, 0.1, 0.01, 0.01, 0.05])
    t, s = _handles("small", map_neighbourhood=7)
    with t, s:
        before = t.align_map(s, d["init"])
        calls = {
            "search_map": lambda: t.search_map(s, *window),
            "search_align_map": lambda: t.search_align_map(s, *window),
            "score_map_poses": lambda: t.score_map_poses(s, poses, with_hits=True),
            "best_map_poses": lambda: t.best_map_poses(s, poses),
            "best_map_poses_align": lambda: t.best_map_poses_align(s, poses),
        }
        for name, call in calls.items():
            with pytest.raises(L.NdtError) as err:
                call()
            assert err.value.code == L.NDT_ERR_INVALID_ARG, name
            assert "ndt3d_set_map_neighbourhood" in str(err.value), (name, str(err.value))
        assert _same(t.align_map(s, d["init"]), before)            # the handle works afterwards
        s.set_map_neighbourhood(7)                                 # a source at 7 is no reason to refuse
        t.set_map_neighbourhood(1)
        for name, call in calls.items():
            out = call()
            assert out is not None and len(out) > 0, name


def test_a_reloaded_submap_aligns_as_the_live_one(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = _pair("small")
    t, s = _handles("small", map_neighbourhood=7)
    with t, s, NdtMatcher3D(cell_size=1.0, map_neighbourhood=7) as t2, NdtMatcher3D(cell_size=1.0) as s2:
        t2.load_map(t.save_map())
        s2.load_map(s.save_map())
        assert t2.map_neighbourhood == 7                           # the handle's setting, not the map's: load keeps it
        want_a, want_e = t.align_map(s, d["init"]), t.evaluate_map(s, d["init"])
        assert want_e[3] == 196
        for tt, ss in ((t2, s), (t, s2), (t2, s2)):
            assert _same(tt.align_map(ss, d["init"]), want_a) and _same_eval(tt.evaluate_map(ss, d["init"]), want_e)


def test_the_map_pyramid_sets_every_level(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMapPyramid3D
    d = _pair("small")
    t, s = _handles("small")
    with t, s:
        p7, p1, ps = NdtMapPyramid3D(t, map_neighbourhood=7), NdtMapPyramid3D(s), None
        try:
            assert [m.map_neighbourhood for m in p7.levels] == [7] * len(p7.levels) and t.map_neighbourhood == 7
            assert [m.map_neighbourhood for m in p1.levels] == [1] * len(p1.levels)
            r = p7.align_map(p1, d["init"])
            assert r.status in (L.NDT_OK, L.NDT_NOT_CONVERGED) and r.n_hit > 0
            ps = NdtMapPyramid3D.from_blob(s.save_map(), map_neighbourhood=7)
            assert [m.map_neighbourhood for m in ps.levels] == [7] * len(ps.levels)
        finally:
            for p in (p7, p1, ps):
                if p is not None:
                    p.close()
