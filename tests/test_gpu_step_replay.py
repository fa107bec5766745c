"""Every device Gauss-Newton step against the float64 oracle, from the doubles the device fed its own solver.

gn_update / solve3 (csrc/ndt2d_kernels.hpp) and gn_update3 / solve6 (csrc/ndt3d_kernels.hpp) - LDL^T with fast_rcp
reciprocals, the 12-rung Levenberg ladder, the step limits, the angle wrap, the line-search state machine and the stop
rule - are inlined into every alignment driver.  A result row holds H, g, score and n_hit of the evaluation behind its
update as doubles, so the oracle's update from the row before's pose must land on the row's pose to the accuracy of a
float64 solve (tests/step_replay.py: step_tolerance, C_STEP from the oracle's own measured error), with the same
iteration count, status and stop.  The float32 evaluation noise that sets the 1e-4 of the trajectory tests cancels.

Trace replays walk ndt2d/ndt3d_align_trace (k_iterate / k_iterate3) through the cases of step_replay.CASES2D / CASES3D;
one-step replays (fixed_iterations = 1: H, g are those of the evaluation at the wrapped initial pose) reach the drivers
without a trace.  A stop is accepted either way only where a deciding norm lies within 1e-9 (relative) of eps_trans /
eps_rot; tests/test_step_replay.py shows that the oracle's cases stay 1e6 times clear of that margin.

What a wrong solver looks like here (emulated on the CPU: a mutated copy of the oracle's update produced the rows,
check_rows judged them): reciprocals 27 eps off, as from a Newton step too few in fast_rcp, fail the Newton far start
and the tight-limits trace; a rotation limit tested on the step before the translation limit shortened it fails row 4
of the tight-limits trace by 4 mm; a stop rule on the unscaled step ends the line-search case one row early.  The
final poses of all three stay within 1e-5 of the right ones, inside the 1e-4 of the trajectory tests."""
import numpy as np
import pytest

import step_replay as S

pytestmark = pytest.mark.gpu

ALL = [(2, n) for n in S.CASES2D] + [(3, n) for n in S.CASES3D]
SPLIT_FROM = S.SPLIT_FROM


_api = S.device_api


@pytest.mark.parametrize("dim,name", ALL, ids=[f"{d}d-{n}" for d, n in ALL])
def test_trace_replays_step_by_step(gpu_lib, dim, name):
    Matcher, _, params, replay, tk, sk = _api(dim)
    pair, start, opt, want = (S.CASES2D if dim == 2 else S.CASES3D)[name]
    d, init = pair(), tuple(start())
    with Matcher(**opt) as m:
        m.set_target(*[d[k] for k in tk])
        rows = m.align_trace(*[d[k] for k in sk], init, capacity=128)
    prm = params(**opt)
    rep = replay(init, rows, prm)
    print(f"\n{dim}D {name}: {len(rows)} rows, status {rows[-1].status}, rungs {[r['rung'] for r in rep][:16]}, "
          f"reached {sorted(S.reached(rep, rows, prm))}")
    S.check_rows(rep, rows, prm, f"{dim}D {name}")
    assert set(want) <= S.reached(rep, rows, prm), (want, [(r["kind"], r["rung"], r["limit"]) for r in rep])


_one_step_results = S.one_step_results


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("name", S.ONE_STEP)
def test_one_update_of_every_driver_replays(gpu_lib, dim, name):
    _, _, params, replay, _, _ = _api(dim)
    failures, seen = [], []
    for label, r, init, kw, own in _one_step_results(dim, name):
        prm = params(**kw)
        rep = replay(init, [r], prm)
        seen.append((label, r.status, r.n_hit, rep[0]["kind"], rep[0]["rung"], rep[0]["limit"]))
        try:
            S.check_rows(rep, [r], prm, label)
            assert rep[0]["kind"] == "step" and r.iterations == 1 and r.status == 0, "no step taken"
            if own and name == "newton_far":
                assert rep[0]["rung"] >= 5, "the Newton far start must climb the ladder"
            if own and name == "tight_limits":
                assert rep[0]["limit"] in ("trans", "rot"), "the tight limits must scale the step"
        except AssertionError as e:
            failures.append((label, str(e)[:600]))
    print(f"\n{dim}D {name}:")
    for row in seen:
        print("   ", row)
    assert not failures, failures
    # single-pair kernels + starts and scans of the two multi calls + batch variants + map-to-map
    assert len(seen) == (4 if dim == 2 else 1) + 2 * (2 + SPLIT_FROM) + (3 if dim == 2 else 2) + 1


def test_one_point_sources_climb_the_ladder_on_the_device(gpu_lib):
    """One source point, min_hits = 1: a Hessian of rank 2.  Through k_align_small and k_iterate, one update each: where
    the device reports NDT_OK the replay agrees on the pose, where the oracle - from the device's own H - says degenerate
    so does the device.  The first 16 points of the source one at a time (float32 terms: singular to 1e-8, rung 0 with a
    condition number of 1e8 or a higher rung, as rounding has it; two of them miss the map: NDT_TOO_FEW_HITS, pose
    untouched), and the point at the origin of the source frame, singular exactly: rung >= 1 for certain.  Then the
    whole loop on that one and on the first through the trace."""
    from gtsam_ndt_amd import _lib as L
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = S.pair2d()
    pairs = [("origin", S.origin_point_pair())] + [(f"point {i}", S.one_point_pair(i)) for i in range(16)]
    opt = pairs[0][1][3]
    kw = dict(opt, fixed_iterations=1)
    prm = S.params2d(**kw)
    for driver, tuning in (("k_align_small", {}), ("k_iterate", {"short_scan_kernel": 0})):
        rungs, kappa = {}, 0.0
        with NdtMatcher2D(tuning=tuning, **kw) as m:
            m.set_target(d["tx"], d["ty"])
            for label, (sx, sy, init, _) in pairs:
                r = m.align(sx, sy, init)
                rep = S.replay2d(init, [r], prm)
                if rep[0]["status"] == L.NDT_DEGENERATE_HESSIAN:
                    assert r.status == L.NDT_DEGENERATE_HESSIAN, (driver, label)
                    continue
                S.check_rows(rep, [r], prm, f"{driver}, {label}")
                rungs[label] = rep[0]["rung"]
                if rep[0]["kind"] == "step" and np.any(rep[0]["applied"]):       # (a point too far to weigh: H = 0, no step)
                    kappa = max(kappa, S.scaled_condition(r.H, rep[0]["rung"]))
        print(f"\none point, {driver}: rungs {rungs}, largest scaled condition number {kappa:.3g}")
        assert rungs["origin"] >= 1
        assert sum(1 for v in rungs.values() if v is not None) >= 12 and kappa > 1e5
    prm = S.params2d(**opt)
    with NdtMatcher2D(**opt) as m:
        m.set_target(d["tx"], d["ty"])
        for label, (sx, sy, init, _) in pairs[:2]:
            rows = m.align_trace(sx, sy, init, capacity=128)
            rep = S.replay2d(init, rows, prm)
            S.check_rows(rep, rows, prm, f"trace, {label}")


def test_3d_newton_rows_carry_the_newton_hessian(gpu_lib):
    """The contract (include/ndt_hip.h) says a row's H is the form hessian_mode selects: in 3D that is the sums after
    newton_rot_block3, not the Gauss-Newton part.  Row 0 of every point-to-map driver, against the oracle's two forms at
    the same pose: ten times closer to the Newton one."""
    from oracle import ndt3d as o3
    d = S.pair3d()
    seen = 0
    for label, r, init, kw, own in _one_step_results(3, "newton_far"):
        if not own:
            continue
        g = o3.build_grid3(d["tx"], d["ty"], d["tz"], S.params3d(**kw))
        pose = tuple(init[:3]) + tuple(S.o2.wrap_angle(v) for v in init[3:])
        Hn = o3.evaluate3(g, d["sx"], d["sy"], d["sz"], pose, S.params3d(**kw), mirror32=True)[0]
        Hg = o3.evaluate3(g, d["sx"], d["sy"], d["sz"], pose, S.params3d(**dict(kw, hessian_mode=0)), mirror32=True)[0]
        sc = np.sqrt(np.outer(np.diag(Hg), np.diag(Hg)))
        e_newton, e_gn = np.max(np.abs(r.H - Hn) / sc), np.max(np.abs(r.H - Hg) / sc)
        assert e_gn > 0.05 and e_newton < 0.1 * e_gn, (label, e_newton, e_gn)
        seen += 1
    assert seen >= 1 + 2 * (2 + SPLIT_FROM) + 1
