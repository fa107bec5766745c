"""Every SE(3) path of the device at steep roll and pitch against the float64 referees (tests/tilted_cases.py).

The device carries four separately derived forms of the derivatives of R = Rz Ry Rx: the Jacobian form (make_rot3 +
accumulate_point3: k_iterate3, evaluate, the multi-start and multi-scan chains), the second derivatives
(newton_rot_block3: every Newton-mode driver), the map-frame form (accumulate_point3_map + map_sums_to_pose_frame: both
k_batch3 variants) and the map-to-map form (make_map_pose3, axis_cross, rot_terms3, accumulate_component3: align_map,
evaluate_map).  Every other test keeps |roll|, |pitch| <= 0.05 rad, where a wrong sin roll * sin pitch term or a roll
axis formed without the pitch is worth less than the tolerances (tests/test_tilted_ref.py emulates three such slips:
they pass there and miss by 4 to 2000 bounds here).  On tilted_cases.ATTITUDES - "steep" (0.7, -0.5, 2.1), "inverted"
(-2.4, 1.1, -0.9), "near_gimbal" (1.2, 1.45, 0.4) - the golden 4096-point pair, its source re-expressed, one target grid
per cell size:

 (a) evaluate and evaluate_map against evaluate3(mirror32) / d2d3_ref.evaluate;
 (b) one update of every alignment driver (step_replay.one_step_results): the row replays through the oracle's update,
     and - what the step replay cannot see - its H, g, score and n_hit are the oracle's at the start pose;
 (c) align_trace replays step by step, default options, tight limits and line search;
 (d) converged poses of every driver against the float64 reference, multi calls bit for bit their single calls;
 (e) one update at pitch = pi / 2 exactly, where H has rank 5.

Bounds: tilted_cases.judge_eval = those of test_evaluate3d_parity (n_hit 3, Jacobi-scaled H 2e-4, score 2e-4, g 1e-3 of
sqrt(H_ii score)); map-to-map: d2d3_ref.eval_bounds on this file's own poses (4 x the restatement's own float32 error,
floored at 2e-5); poses: 1e-4 m and 1e-4 in rot_gap against references admitted by test_tilted_ref.py.

Measured on one MI355X, worst over the attitudes and poses (the prints of this file give every figure):
                                              n_hit   H        score    g        bound (H, score, g)
  (a) evaluate, Gauss-Newton                  equal   1.9e-6   4.4e-7   5.3e-7   2e-4, 2e-4, 1e-3
      evaluate, Newton                        equal   5.4e-6   4.4e-7   5.3e-7
      Newton rotation block (Newton - Gauss-Newton H), k_iterate3 and 12 starts 7.8e-7, batch3 2.7e-6; bound 2e-5
      evaluate_map, 1 m and 2 m, both forms   equal   2.9e-5   1.2e-6   7.7e-6   eval_bounds: 2e-5 .. 1.1e-4, 2e-5, 2e-5 .. 3e-5
  (b) k_iterate3                              equal   2.2e-5   4.8e-7   2.0e-6   2e-4, 2e-4, 1e-3
      align_multi_start / _scan, 2 and 12     equal   3.7e-5   6.5e-7   3.5e-6
      batch3 on chip                          equal   2.2e-5   4.7e-7   2.0e-6
      batch3 global tables (0.75 m)           equal   2.4e-5   7.3e-7   3.3e-6
      align_map (vs d2d3_ref)                 equal   9.2e-6   1.2e-6   4.4e-6   eval_bounds at the start pose
      the largest H figures are the Newton rows from the far start ("inverted", 12 starts: 3.7e-5)
  (c) nine traces of 30 to 40 rows replay; "steep" with line search rejects no trial, on the device as in the oracle
  (d) converged poses: status and iteration count equal to the reference's in every case (32 / 39 / 40 Gauss-Newton,
      97 / 33 / 68 at 0.75 m, 4 Newton, 8 to 16 map-to-map); translation <= 3.2e-7 m, rot_gap <= 7.3e-8 (bound 1e-4)
  (e) pitch = pi / 2: every driver steps at rung 0 or 1 (a matter of rounding, as the start moves a millimetre), scaled
      condition number up to 8.1e7; no driver and no replay calls the Hessian degenerate.
No kernel had to change: the four forms agree with the referees at every attitude."""
import math

import numpy as np
import pytest

import d2d3_ref as R
import step_replay as S
import tilted_cases as T
from oracle import ndt3d as o3

pytestmark = pytest.mark.gpu

NAMES = sorted(T.ATTITUDES)
SRC = ("sx", "sy", "sz")
TGT = ("tx", "ty", "tz")


def _matcher(**kw):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = S.pair3d()
    m = NdtMatcher3D(**kw)
    m.set_target(*[d[k] for k in TGT])
    return m


def _src(d):
    return [d[k] for k in SRC]


def _map_handles(name, **kw):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    t, s = _matcher(**kw), NdtMatcher3D(**kw)
    s.set_target(*_src(T.tilted_pair(name)))
    return t, s


_maps = {}


def _ref_maps(name, cell):
    if (name, cell) not in _maps:
        d = T.tilted_pair(name)
        _maps[name, cell] = (T.grid(cell), R.build_map(d["sx"], d["sy"], d["sz"], o3.Ndt3Params(cell_size=cell))[1])
    return _maps[name, cell]


def _judge_map(got, name, cell, pose, mode, bound=None):
    """An evaluation of the map-to-map objective against the restatement: test_evaluate_map_matches_the_restatement's
    rule; the bound from this very pose unless given."""
    tgt, comps = _ref_maps(name, cell)
    prm = o3.Ndt3Params(cell_size=cell, hessian_mode=mode)
    if bound is None:
        bound = R.eval_bounds([(tgt, comps, pose)], prm)[0]
    ref = R.evaluate(tgt, comps, pose, prm)
    diffs = R.eval_diffs(got, ref, R.evaluate(tgt, comps, pose, o3.Ndt3Params(cell_size=cell))[0])
    assert got[3] == ref[3] and all(a <= b for a, b in zip(diffs, bound)), (name, cell, mode, got[3], ref[3], diffs, bound)
    return diffs


# ------------------------------------------------------------------------------------------------------ (a) evaluation
@pytest.mark.parametrize("mode", [0, 1], ids=["gauss_newton", "newton"])
@pytest.mark.parametrize("name", NAMES)
def test_evaluate_at_a_tilted_pose(gpu_lib, name, mode):
    d = T.tilted_pair(name)
    w = T.Worst()
    with _matcher(hessian_mode=mode) as m:
        for pose in T.eval_poses(name):
            got = m.evaluate(*_src(d), pose)
            Hgn = T.oracle_eval(d, pose, 0)[0]
            ref = T.oracle_eval(d, pose, mode)
            w.add(f"evaluate {name} mode {mode}", T.eval_figures(got, ref, Hgn))
            T.judge_eval(got, ref, Hgn, (name, mode, pose))
            truth = T.oracle_eval(d, pose, mode, mirror32=False)
            assert abs(got[3] - truth[3]) <= 5 and abs(got[2] - truth[2]) / truth[2] < 5e-3
            if mode == 1:
                # test_3d_newton_rows_carry_the_newton_hessian's rule
                sc = np.sqrt(np.outer(np.diag(Hgn), np.diag(Hgn)))
                e_newton, e_gn = np.max(np.abs(got[0] - ref[0]) / sc), np.max(np.abs(got[0] - Hgn) / sc)
                assert e_gn > 0.05 and e_newton < 0.1 * e_gn, (name, e_newton, e_gn)
    w.report("(a) evaluate vs evaluate3(mirror32)")


def _hessians_at(d, pose, mode):
    """driver -> the H of its evaluation at `pose`: evaluate (k_iterate3), the first and last of 12 starts of the
    two-kernel multi-start chain, and the batch kernel (whose M comes out of the map-frame sums), one update each."""
    from gtsam_ndt_amd.matcher import NdtBatch3D
    kw = dict(hessian_mode=mode, fixed_iterations=1)
    out = {}
    with _matcher(**kw) as m:
        out["k_iterate3"] = m.evaluate(*_src(d), pose)[0]
        rows = m.align_multi_start(*S._cuda(_src(d)), [pose] * S.SPLIT_FROM)
        out["align_multi_start, 12 starts [0]"], out["align_multi_start, 12 starts [11]"] = rows[0].H, rows[-1].H
    with NdtBatch3D(**kw) as b:
        out["batch3, on chip"] = b.align([tuple(S.pair3d()[k] for k in TGT)], [tuple(_src(d))], [pose])[0].H
    return out


@pytest.mark.parametrize("name", NAMES)
def test_newton_rotation_block_at_a_tilted_pose(gpu_lib, name):
    """What newton_rot_block3 and the - d2 (J'v)(J'v)' term add to the rotation block, device (Newton evaluation minus
    Gauss-Newton evaluation of the same driver) against oracle, to 4 x the oracle's own float32 error floored at the
    project's 2e-5: ten times tighter than judge_eval, because the terms that make its noise cancel.  A d2R/dpitch2
    without its u w' term misses this by a factor of six at "steep" and passes judge_eval (tests/test_tilted_ref.py)."""
    d = T.tilted_pair(name)
    poses = T.eval_poses(name)
    bound, own = T.newton_block_bound(d, poses)
    worst = {}
    for pose in poses:
        Hgn = T.oracle_eval(d, pose, 0)[0]
        ref = T.newton_block(T.oracle_eval(d, pose, 1)[0], Hgn, Hgn)
        assert np.abs(ref).max() > 0.05                                      # the block is there to be got wrong
        newton, gn = _hessians_at(d, pose, 1), _hessians_at(d, pose, 0)
        for driver in newton:
            e = float(np.abs(T.newton_block(newton[driver], gn[driver], Hgn) - ref).max())
            worst[driver] = max(worst.get(driver, 0.0), e)
    print(f"\n(a) {name}: Newton rotation block vs the oracle {({k: f'{v:.2e}' for k, v in worst.items()})}; "
          f"the oracle's float32 vs float64 {own:.2e}, bound {bound:.2e}")
    assert len(worst) == 4 and max(worst.values()) <= bound, worst


@pytest.mark.parametrize("cell", [1.0, 2.0])
@pytest.mark.parametrize("mode", [0, 1], ids=["gauss_newton", "newton"])
@pytest.mark.parametrize("name", NAMES)
def test_evaluate_map_at_a_tilted_pose(gpu_lib, name, mode, cell):
    tgt, comps = _ref_maps(name, cell)
    prm = o3.Ndt3Params(cell_size=cell, hessian_mode=mode)
    poses = T.eval_poses(name) + [T.map_start(name)]
    bound, worst = R.eval_bounds([(tgt, comps, p) for p in poses], prm)
    print(f"\n{name} {cell} m mode {mode}: float32 vs float64 of the restatement (H, g, score) {worst}; bound {bound}")
    w = T.Worst()
    t, s = _map_handles(name, cell_size=cell, hessian_mode=mode)
    try:
        for pose in poses:
            got = t.evaluate_map(s, pose)
            w.add(f"evaluate_map {name} {cell} m mode {mode}", _judge_map(got, name, cell, pose, mode, bound))
            assert np.array_equal(got[0], got[0].T) and got[3] >= 100
    finally:
        t.close(); s.close()
    w.report("(a) evaluate_map vs d2d3_ref.evaluate (float64)", ("H", "g", "score"))


# -------------------------------------------------------------------------------------- (b) one update of every driver
@pytest.mark.parametrize("case", S.ONE_STEP)
@pytest.mark.parametrize("name", NAMES)
def test_one_update_of_every_driver_at_a_tilted_pose(gpu_lib, name, case):
    d = T.tilted_pair(name)
    failures, seen, w = [], [], T.Worst()
    for label, r, init, kw, _ in S.one_step_results(3, case, pair=d, init=T.far_start(name)):
        prm = S.params3d(**kw)
        start = T.wrapped(init)
        rep = S.replay3d(init, [r], prm)
        seen.append((label, r.status, r.n_hit, rep[0]["kind"], rep[0]["rung"], rep[0]["limit"]))
        driver = label.split(" [")[0]
        try:
            S.check_rows(rep, [r], prm, label)
            assert rep[0]["kind"] == "step" and r.iterations == 1 and r.status == 0, "no step taken"
            got = (r.H, r.g, r.score, r.n_hit)
            if label == "align_map":
                w.add(f"{driver} {name} {case}", (0,) + tuple(np.array(_judge_map(got, name, 1.0, start, prm.hessian_mode))[[0, 2, 1]]))
                continue
            # a point-to-map driver (the global-table batch on its own 0.75 m grid): the sums behind the step are the
            # oracle's at the start pose
            ref = T.oracle_eval(d, start, prm.hessian_mode, cell_size=prm.cell_size)
            Hgn = T.oracle_eval(d, start, 0, cell_size=prm.cell_size)[0]
            w.add(f"{driver} {name} {case}", T.eval_figures(got, ref, Hgn))
            T.judge_eval(got, ref, Hgn, label)
            if case == "tight_limits":
                assert rep[0]["limit"] in ("trans", "rot"), "the tight limits must scale the step"
        except AssertionError as e:
            failures.append((label, str(e)[:600]))
    print(f"\n{name} {case}:")
    for row in seen:
        print("   ", row)
    w.report("(b) the row's H, g, score, n_hit vs the oracle at the start (align_map: vs d2d3_ref)")
    assert not failures, failures
    assert len(seen) == 1 + 2 * (2 + S.SPLIT_FROM) + 2 + 1


# ------------------------------------------------------------------------------------------------------------ (c) trace
@pytest.mark.parametrize("case", sorted(T.TRACE_CASES))
@pytest.mark.parametrize("name", NAMES)
def test_trace_replays_step_by_step_at_a_tilted_pose(gpu_lib, name, case):
    opt, want = T.trace_case(name, case)
    d, init = T.tilted_pair(name), T.far_start(name)
    with _matcher(**opt) as m:
        rows = m.align_trace(*_src(d), init, capacity=128)
    prm = S.params3d(**opt)
    rep = S.replay3d(init, rows, prm)
    got = S.reached(rep, rows, prm)
    print(f"\n{name} {case}: {len(rows)} rows, status {rows[-1].status}, reached {sorted(got)}")
    S.check_rows(rep, rows, prm, f"{name} {case}")
    assert set(want) <= got, (want, sorted(got))


# -------------------------------------------------------------------------------------------------- (d) converged poses
def _hold_to(r, ref, label, converged_gn=True):
    gap = T.pose_gap(r.pose, ref["pose"])
    print(f"    {label}: device {r.iterations} iterations status {r.status}, reference {ref['iterations']} / {ref['status']}, "
          f"gap {gap[0]:.2e} m {gap[1]:.2e}")
    assert r.status == ref["status"] == 0, label
    assert abs(r.iterations - ref["iterations"]) <= (3 if converged_gn else 2), label
    assert gap[0] < T.POSE_TOL and gap[1] < T.POSE_TOL, (label, gap)
    return gap


def _equal(a, b):
    assert a.status == b.status and a.iterations == b.iterations and a.n_hit == b.n_hit, (a, b)
    assert a.pose == b.pose and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g) and a.score == b.score


@pytest.mark.parametrize("name", NAMES)
def test_converged_poses_at_a_tilted_pose(gpu_lib, name):
    from gtsam_ndt_amd.matcher import NdtBatch3D
    d = T.tilted_pair(name)
    src = _src(d)
    init, ref = T.reference_run(name)
    w = T.Worst()
    print(f"\n{name}:")
    with _matcher() as m:
        single = m.align(*src, init)
        w.add("k_iterate3", _hold_to(single, ref, "single handle"))
        dev = S._cuda(src)
        starts = S._starts(init, 2)
        multi = m.align_multi_scan([dev] * 2, starts)
        for k, r in enumerate(multi):
            _equal(r, m.align(*dev, starts[k]))                          # bit for bit its single-call result
        _equal(multi[0], single)
        ref1 = o3.align3(T.grid(), *src, T.wrapped(starts[1]), o3.Ndt3Params())          # the second scan: 1 mm off the far start
        w.add("align_multi_scan", _hold_to(multi[1], ref1, "align_multi_scan [1]"))
    for label, how, extra in (("batch3, on chip", {}, {}), ("batch3, global tables", dict(global_workgroups=8), S.GLOBAL3D)):
        with NdtBatch3D(**how, **extra) as b:
            r = b.align([tuple(d[k] for k in TGT)], [tuple(src)], [init])[0]
        w.add(label, _hold_to(r, T.reference_run(name, cell_size=extra.get("cell_size", 1.0))[1], label))
    near, refn = T.reference_run(name, 1, "near")
    with _matcher(hessian_mode=1) as m:
        w.add("k_iterate3, Newton", _hold_to(m.align(*src, near), refn, "Newton from the near start", converged_gn=False))
    for cell in (1.0, 2.0):
        tgt, comps = _ref_maps(name, cell)
        start = T.map_start(name)
        refm = R.align(tgt, comps, T.wrapped(start), o3.Ndt3Params(cell_size=cell))
        t, s = _map_handles(name, cell_size=cell)
        try:
            one = t.align_map(s, start)
            w.add(f"align_map {cell} m", _hold_to(one, refm, f"align_map {cell} m"))
            other = S._starts(start, 2)[1]
            multi = t.align_map_multi([s, s], [start, other])            # bit for bit its single calls
            _equal(multi[0], one)
            _equal(multi[1], t.align_map(s, other))
        finally:
            t.close(); s.close()
    w.report(f"(d) {name}: converged pose vs the float64 reference", ("m", "rot_gap"))


# ------------------------------------------------------------------------------------------- (e) the singular attitude
def test_one_update_at_the_singular_attitude(gpu_lib):
    """pitch = pi / 2 exactly: roll and yaw turn about the same axis, the roll and yaw columns of every Jacobian are
    equal up to sign and H has rank 5 - in float64; from float32 terms it is singular to 1e-8 of its scale, and whether
    the last pivot passes at rung 0 is a matter of rounding.  The rule of
    test_one_point_sources_climb_the_ladder_on_the_device, through every driver: where the oracle, from the device's own
    H, says degenerate so does the device, otherwise the replay agrees on the pose; the rung is reported.  The check is
    not vacuous: test_tilted_ref.test_the_singular_attitude_is_worth_judging holds the tolerance of this step below
    1e-5 of the step on the oracle's own H."""
    from gtsam_ndt_amd import _lib as L
    d = T.tilted_pair(T.SINGULAR)
    init = tuple(np.array(d["pose"]) - T.FAR_OFFSET * np.array((1, 1, 1, 1, 0, 1)))          # the pitch stays pi / 2
    assert init[4] == math.pi / 2.0
    rungs, kappa, failures = {}, 0.0, []
    for label, r, start, kw, _ in S.one_step_results(3, "tight_limits", pair=d, init=init):
        prm = S.params3d(**kw)
        rep = S.replay3d(start, [r], prm)
        try:
            if rep[0]["status"] == L.NDT_DEGENERATE_HESSIAN:
                assert r.status == L.NDT_DEGENERATE_HESSIAN, "the oracle says degenerate, the device does not"
                continue
            S.check_rows(rep, [r], prm, label)
            assert rep[0]["kind"] == "step" and r.status == 0
            rungs[label] = rep[0]["rung"]
            kappa = max(kappa, S.scaled_condition(r.H, rep[0]["rung"]))
            if label != "align_map":
                ref = T.oracle_eval(d, T.wrapped(start), 0, cell_size=prm.cell_size)
                T.judge_eval((r.H, r.g, r.score, r.n_hit), ref, label=label)
        except AssertionError as e:
            failures.append((label, str(e)[:600]))
    print(f"\npitch = pi / 2: rungs {rungs}, largest scaled condition number {kappa:.3g}")
    assert not failures, failures
    assert len(rungs) >= 16 and kappa > 1e4
