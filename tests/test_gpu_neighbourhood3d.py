"""ndt3d_set_neighbourhood(h, 7): a source point is scored against its own voxel and the six face neighbours
(docs/ALGORITHM.md 2.25), on every alignment chain, against the float64 restatement tests/ndt3d_nb_ref.py.

Hand-built grids (one 8 x 8 x 8 reserved extent at cell 1, origin 0, a few voxels filled) pin which voxels count: faces
only, by index and never by key arithmetic, nothing for a point outside the grid.  The seeded lidar pair pins the sums,
the alignment, every chain bit for bit against the single call, the switch on one handle (a stale cached graph would
show there), the untouched default and the refusals.  3D handles have no NDT_TUNE_LAUNCH_GRAPHS and no
NDT_TUNE_SPLIT_FROM (ndt3d_set_tuning refuses both): the chains run under both settings of NDT_TUNE_FUSED_BEGIN, and
align_trace is the plain-launch path."""
import numpy as np
import pytest

from gtsam_ndt_amd import synth3d

import ndt3d_nb_ref as N

pytestmark = pytest.mark.gpu

ZERO = (0.0,) * 6
FIELDS = ("pose", "score", "iterations", "n_hit", "status")


def same(a, b):
    return all(getattr(a, f) == getattr(b, f) for f in FIELDS) and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g)


def same_eval(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and a[3] == b[3]


# ------------------------------------------------------------------------------------------------- hand-built grids
def hand_matcher(voxels, seed=5, **kw):
    """A matcher over [0, 8)^3 at cell 1 with 16 points scattered over each of `voxels` (index triples; spread over the
    whole voxel, so that the centre of a neighbour still scores 1e-5 .. 1e-2 of d1, a normal float32), and the grid
    it holds as the restatement's Grid3D: the device's own float32 records, so that only the scoring is compared.  A
    voxel's points depend on the seed and the voxel alone, so a voxel has the same record in every grid it is part of."""
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    from oracle import ndt3d as o
    m = NdtMatcher3D(**kw)
    info = m.reserve_target((1.0, 1.0, 1.0), (6.5, 6.5, 6.5))
    assert (info.ox, info.oy, info.oz) == (0.0, 0.0, 0.0) and (info.width, info.height, info.depth) == (8, 8, 8)
    pts = np.concatenate([np.array(v) + 0.5 + np.random.default_rng([seed, *v]).uniform(-0.49, 0.49, size=(16, 3))
                          for v in voxels]).astype(np.float32)
    assert m.add_target_points(pts[:, 0].copy(), pts[:, 1].copy(), pts[:, 2].copy()) == 0
    count, mean, icov = m.grid()
    valid = icov[:, 0] != 0
    assert int(valid.sum()) == len(voxels) == m.grid_info().n_valid
    g = o.Grid3D(np.zeros(3, np.float32), np.float32(info.inv_cell), (8, 8, 8), count.astype(np.int64),
                 mean.astype(np.float64), icov.astype(np.float64), valid, int(valid.sum()))
    return m, g


def one_point(m, p, nb):
    """(score, n_hit) of the single source point p at the identity under neighbourhood nb"""
    m.set_neighbourhood(nb)
    p = np.asarray(p, np.float32)
    H, g, s, nh = m.evaluate(p[0:1].copy(), p[1:2].copy(), p[2:3].copy(), ZERO)
    return s, nh


def ref_point(g, p, nb):
    from oracle import ndt3d as o
    p = np.asarray(p, np.float32)
    r = N.evaluate3_nb(g, p[0:1], p[1:2], p[2:3], ZERO, o.Ndt3Params(), nb, mirror32=True)
    return r[2], r[3]


def test_faces_only(gpu_lib):
    V = np.array([3, 3, 3])
    m, g = hand_matcher([V])
    with m:
        for d in ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1)):
            p = V + 0.5 + np.array(d)
            assert one_point(m, p, 1) == (0.0, 0)
            s, nh = one_point(m, p, 7)
            sr, nr = ref_point(g, p, 7)
            assert nh == nr == 1 and 0.0 < sr < 1.0 and abs(s - sr) <= 2e-4 * sr, (d, s, sr)
        for d in ((1, 1, 0), (-1, 0, 1), (0, -1, -1), (1, 1, 1), (-1, 1, -1)):          # edge and corner neighbours
            p = V + 0.5 + np.array(d)
            assert one_point(m, p, 1) == (0.0, 0) and one_point(m, p, 7) == (0.0, 0), d
    m2, g2 = hand_matcher([V, V + np.array([1, 0, 0])])
    with m2:
        p = V + np.array([0.7, 0.4, 0.55])
        s1, n1 = one_point(m2, p, 1)
        s7, n7 = one_point(m2, p, 7)
        (r1, k1), (r7, k7) = ref_point(g2, p, 1), ref_point(g2, p, 7)
        assert (n1, n7) == (k1, k7) == (1, 2)
        assert abs(s1 - r1) <= 2e-4 * r1 and abs(s7 - r7) <= 2e-4 * r7
        # the sum of the two single-voxel terms: the second one is what a point scores at 7 with only the +x voxel there
        m3, _ = hand_matcher([V + np.array([1, 0, 0])])
        with m3:
            s_x, n_x = one_point(m3, p, 7)
        assert n_x == 1 and abs(s7 - (s1 + s_x)) <= 4e-7 * s7          # two float32 terms, added in float32


def test_no_wrap_and_nothing_for_points_outside(gpu_lib):
    """Each point lies in a border voxel, and the voxel that key -/+ 1, W reaches from there (the far end of the row or
    layer before / after) is valid; key -/+ W H from iz = 0 / D - 1 is no voxel at all.  None of them is a neighbour."""
    cases = [((0, 3, 1), (7, 2, 1)), ((7, 3, 5), (0, 4, 5)), ((3, 0, 3), (3, 7, 2)), ((5, 7, 6), (5, 0, 7)),
             ((3, 3, 0), None), ((3, 3, 7), None)]
    m, g = hand_matcher([v for _, v in cases if v is not None])
    with m:
        for at, reached in cases:
            p = np.array(at) + 0.5
            assert one_point(m, p, 7) == (0.0, 0) and ref_point(g, p, 7) == (0.0, 0), at
            if reached is not None:                                    # ... and the voxel it must not reach does score
                assert one_point(m, np.array(reached) + 0.5, 7)[1] == 1
        # a quarter cell past a face, next to the valid voxel (7, 2, 1); and a NaN point
        assert one_point(m, (8.25, 2.5, 1.5), 7) == (0.0, 0) and one_point(m, (7.75, 2.5, 1.5), 7)[1] == 1
        assert one_point(m, (-0.25, 4.5, 5.5), 7) == (0.0, 0)
        assert one_point(m, (np.nan, 2.5, 1.5), 7) == (0.0, 0) and one_point(m, (6.5, 2.5, np.nan), 7) == (0.0, 0)
        # among other points too: the scan's sums are those of its inside points
        scan = np.array([[6.5, 2.5, 1.5], [8.25, 2.5, 1.5], [np.nan, 2.5, 1.5], [7.5, 3.5, 1.5]], np.float32)
        H, gr, s, nh = m.evaluate(scan[:, 0].copy(), scan[:, 1].copy(), scan[:, 2].copy(), ZERO)
        sa, sb = one_point(m, scan[0], 7), one_point(m, scan[3], 7)
        assert nh == 2 == sa[1] + sb[1] and abs(s - (sa[0] + sb[0])) <= 4e-7 * s and np.all(np.isfinite(H)) and np.all(np.isfinite(gr))


# ------------------------------------------------------------------------------------------------- the seeded pair
@pytest.fixture(scope="module")
def pair():
    """make_pair3d(6, 256): 1536 points, 6 workgroups' worth.  tests/test_ndt3d_nb_ref.py checks without a device that no
    point of it lies within 4 float32 ulps of a voxel face at either pose and that 7 scores 3.5 hits per hit of 1."""
    import torch
    from oracle import ndt3d as o
    d = synth3d.make_pair3d(n_elev=6, n_azim=256)
    S = (d["sx"], d["sy"], d["sz"])
    dev = tuple(torch.from_numpy(a).cuda() for a in S)
    return d, S, dev, o.build_grid3(d["tx"], d["ty"], d["tz"], o.Ndt3Params())


def matcher(d, nb=1, **kw):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    m = NdtMatcher3D(**kw) if nb == 1 else NdtMatcher3D(neighbourhood=nb, **kw)
    m.set_target(d["tx"], d["ty"], d["tz"])
    return m


@pytest.mark.parametrize("mode", [0, 1])
def test_parity_with_the_restatement(gpu_lib, pair, mode):
    """The bounds of test_gpu_ndt3d.py::test_evaluate3d_parity for the single-voxel form.  The scale of an entry is the
    Gauss-Newton diagonal, as there: the Newton diagonal is negative in yaw at `init` on this scene and sets no scale."""
    from oracle import ndt3d as o
    d, S, _, g = pair
    prm = o.Ndt3Params(hessian_mode=mode)
    with matcher(d, 7, hessian_mode=mode) as m:
        assert m.neighbourhood == 7
        for pose in (d["init"], d["pose"]):
            H, gr, s, nh = m.evaluate(*S, pose)
            Hm, gm, sm, nm, n_border = N.evaluate3_nb(g, *S, pose, prm, 7, mirror32=True)
            print(f"mode {mode}: n_hit {nh} ref {nm} n_border {n_border} score {s} ref {sm}")
            assert n_border <= 3
            assert abs(nh - nm) <= 7 * n_border
            dg = np.diag(Hm) if mode == 0 else np.diag(N.evaluate3_nb(g, *S, pose, o.Ndt3Params(), 7, mirror32=True)[0])
            assert np.all(dg > 0)
            print("  H", np.max(np.abs(H - Hm) / np.sqrt(np.outer(dg, dg))), "score", abs(s - sm) / sm,
                  "g", np.max(np.abs(gr - gm) / np.sqrt(dg * sm)))
            assert np.max(np.abs(H - Hm) / np.sqrt(np.outer(dg, dg))) < 2e-4
            assert abs(s - sm) / sm < 2e-4
            assert np.max(np.abs(gr - gm) / np.sqrt(dg * sm)) < 1e-3
            m.set_neighbourhood(1)
            n1 = m.evaluate(*S, pose)[3]
            m.set_neighbourhood(7)
            assert nh > 1.5 * n1 > 0


def test_align_parity(gpu_lib):
    """The scene and bounds of test_gpu_ndt3d.py::test_align3d_converged_pose_parity (BASELINE.json: 1e-4 m / 1e-4 rad)."""
    from oracle import ndt3d as o
    d = synth3d.make_pair3d(n_elev=32, n_azim=512)
    S = (d["sx"], d["sy"], d["sz"])
    prm = o.Ndt3Params()
    ref = N.align3_nb(o.build_grid3(d["tx"], d["ty"], d["tz"], prm), *S, d["init"], prm, 7)
    with matcher(d, 7) as m:
        r = m.align(*S, d["init"])
        r2 = m.align(*S, d["init"])
        rows = m.align_trace(*S, d["init"])
    assert r.status == ref["status"] == 0
    e = np.abs(np.array(r.pose) - np.array(ref["pose"]))
    print("pose error", e, "iterations", r.iterations, ref["iterations"])
    assert e[:3].max() < 1e-4 and e[3:].max() < 1e-4
    assert abs(r.iterations - ref["iterations"]) <= 3
    assert same(r, r2)
    assert len(rows) == r.iterations and rows[-1].pose == r.pose and rows[-1].status == r.status


def _starts(d, count):
    rng = np.random.default_rng(11)
    return [tuple(np.array(d["init"]) + rng.uniform(-1, 1, 6) * np.array([0.3, 0.3, 0.1, 0.01, 0.01, 0.05])) for _ in range(count)]


@pytest.mark.parametrize("fused_begin", [1, 0])
@pytest.mark.parametrize("fixed", [0, 5])
def test_every_chain_equals_the_single_call(gpu_lib, pair, fused_begin, fixed):
    import torch
    d, S, dev, _ = pair
    starts = _starts(d, 13)
    with matcher(d, 7, fixed_iterations=fixed, tuning={"fused_begin": fused_begin}) as m:
        single = [m.align(*dev, p) for p in starts]
        assert any(r.iterations > 1 for r in single) and all(r.n_hit > 0 for r in single)
        for count in (1, 3, 13):
            rs = m.align_multi_start(*dev, starts[:count])
            assert all(same(a, b) for a, b in zip(rs, single)), count
        # three different scans: the scan, its first 1000 points, and every other point
        scans = [dev, tuple(c[:1000].contiguous() for c in dev), tuple(c[::2].contiguous() for c in dev)]
        rs = m.align_multi_scan(scans, starts[:3])
        for k in range(3):
            assert same(rs[k], m.align(*scans[k], starts[k])), k
        m.align_async(*dev, starts[2])
        assert same(m.finish(), single[2])
        assert same(m.align(*S, starts[2]), single[2])                # host arrays
        torch.cuda.synchronize()


def test_switching_on_one_handle(gpu_lib, pair):
    """A graph cached for one neighbourhood must not be replayed for the other."""
    d, S, dev, _ = pair
    starts = _starts(d, 3)
    with matcher(d, 1, fixed_iterations=5) as m, matcher(d, 7, fixed_iterations=5) as fresh:
        a = m.align(*dev, d["init"])
        am = m.align_multi_start(*dev, starts)
        m.set_neighbourhood(7)
        assert m.neighbourhood == 7
        b = m.align(*dev, d["init"])
        bm = m.align_multi_start(*dev, starts)
        m.set_neighbourhood(1)
        assert m.neighbourhood == 1
        a2 = m.align(*dev, d["init"])
        am2 = m.align_multi_start(*dev, starts)
        assert same(a2, a) and not same(b, a) and b.n_hit > 1.5 * a.n_hit
        assert same(b, fresh.align(*dev, d["init"]))
        assert all(same(x, y) for x, y in zip(am2, am)) and not any(same(x, y) for x, y in zip(bm, am))
        assert all(same(x, y) for x, y in zip(bm, fresh.align_multi_start(*dev, starts)))


def test_the_default_is_untouched(gpu_lib, pair):
    """A handle that never saw the setter and one set to 7 and back to 1: the same bits on the alignment paths and on
    the entry points that 7 refuses.  (The only test here that passes without the option's kernels.)"""
    d, S, dev, _ = pair
    window = (d["pose"], (0.5, 0.5, 0.1), (0.25, 0.25, 0.05))
    poses = np.array(_starts(d, 5))
    with matcher(d) as plain, matcher(d) as toggled:
        if hasattr(toggled, "set_neighbourhood"):
            toggled.set_neighbourhood(7)
            toggled.align(*dev, d["init"])
            toggled.set_neighbourhood(1)
        for m in (plain, toggled):
            assert getattr(m, "neighbourhood", 1) == 1
        assert same_eval(plain.evaluate(*S, d["pose"]), toggled.evaluate(*S, d["pose"]))
        assert same(plain.align(*dev, d["init"]), toggled.align(*dev, d["init"]))
        ha, hb = plain.search_align(*dev, *window, k=3), toggled.search_align(*dev, *window, k=3)
        assert len(ha) == len(hb) > 0
        for (h1, r1), (h2, r2) in zip(ha, hb):
            assert h1.pose == h2.pose and h1.score == h2.score and same(r1, r2)
        assert np.array_equal(plain.score_poses(*S, poses), toggled.score_poses(*S, poses))


def test_refusals(gpu_lib, pair):
    import torch
    from gtsam_ndt_amd import _lib as L
    d, S, dev, _ = pair
    window = (d["pose"], (0.5, 0.5, 0.1), (0.25, 0.25, 0.05))
    poses = np.array(_starts(d, 5))
    dposes = torch.from_numpy(poses).cuda()
    with matcher(d, 7) as m, matcher(d) as other:
        before = m.align(*dev, d["init"])
        calls = {
            "search": lambda: m.search(*S, *window),
            "search_dev": lambda: m.search(*dev, *window),
            "search_scores_dev": lambda: m.search_scores(*dev, *window),
            "search_align_dev": lambda: m.search_align(*dev, *window),
            "score_poses": lambda: m.score_poses(*S, poses),
            "score_poses_dev": lambda: m.score_poses(*dev, dposes),
            "best_poses_dev": lambda: m.best_poses(*dev, dposes),
            "best_poses_align_dev": lambda: m.best_poses_align(*dev, dposes),
            "score_particles": lambda: m.score_particles(*S, poses, with_hits=True),
            "score_particles_dev": lambda: m.score_particles(*dev, dposes),
            "score_particles_async": lambda: m.score_particles(*dev, dposes, sync=False),
            "fit_points": lambda: m.fit_points(*S, d["pose"], 9.0),
            "fit_points_dev": lambda: m.fit_points(*dev, d["pose"], 9.0),
            "select_points_dev": lambda: m.select_points(*dev, d["pose"], 9.0),
        }
        for name, call in calls.items():
            with pytest.raises(L.NdtError) as err:
                call()
            assert err.value.code == L.NDT_ERR_INVALID_ARG, name
            msg = gpu_lib.ndt_last_error().decode()
            assert msg and "neighbourhood" in msg, (name, msg)
        assert same(m.align(*dev, d["init"]), before)
        with pytest.raises(L.NdtError) as err:
            m.set_neighbourhood(3)
        assert err.value.code == L.NDT_ERR_INVALID_ARG and "neighbourhood" in gpu_lib.ndt_last_error().decode()
        assert m.neighbourhood == 7 and same(m.align(*dev, d["init"]), before)
        # with 1 they answer again
        m.set_neighbourhood(1)
        assert all(callable(c) and c() is not None for c in calls.values())
        # map-to-map scores components, not points: the same bits whatever either handle's neighbourhood
        near = tuple(np.array(ZERO) + np.array([0.05, -0.03, 0.01, 0.0, 0.0, 0.01]))
        want_a, want_e = m.align_map(other, near), m.evaluate_map(other, near)
        for nb_t, nb_s in ((7, 1), (1, 7), (7, 7)):
            m.set_neighbourhood(nb_t)
            other.set_neighbourhood(nb_s)
            assert same(m.align_map(other, near), want_a) and same_eval(m.evaluate_map(other, near), want_e)


def test_the_pyramid_sets_every_level(gpu_lib, pair):
    from gtsam_ndt_amd.matcher import NdtPyramid3D
    d, S, _, _ = pair
    with NdtPyramid3D(neighbourhood=7) as p, NdtPyramid3D() as q:
        assert [m.neighbourhood for m in p.levels] == [7] * len(p.levels)
        assert [m.neighbourhood for m in q.levels] == [1] * len(q.levels)
        p.set_target(d["tx"], d["ty"], d["tz"])
        q.set_target(d["tx"], d["ty"], d["tz"])
        rp, rq = p.align(*S, d["init"]), q.align(*S, d["init"])
        assert rp.n_hit > 1.5 * rq.n_hit > 0
