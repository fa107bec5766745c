"""The step-replay helper on the oracle alone (no GPU): replaying the oracle's own traces is exact, the constant of
step_tolerance is what the oracle's measured error says, and every case of tests/step_replay.py reaches the branch the GPU
file (tests/test_gpu_step_replay.py) needs it for."""
import math

import numpy as np
import pytest

import step_replay as S
from oracle import ndt2d as o2
from oracle import ndt3d as o3

ALL = [(2, n) for n in S.CASES2D] + [(3, n) for n in S.CASES3D]
IDS = [f"{d}d-{n}" for d, n in ALL]


def _one_point_rows(pair=S.one_point_pair):
    sx, sy, init, opt = pair()
    d = S.pair2d()
    prm = S.params2d(**opt)
    rows = S.oracle_rows2d(o2.build_grid(d["tx"], d["ty"], prm), sx, sy, init, prm)
    return prm, init, rows, S.replay2d(init, rows, prm)


@pytest.mark.parametrize("dim,name", ALL, ids=IDS)
def test_replay_reproduces_the_oracle_bit_for_bit(dim, name):
    """Both Hessian forms, line_search = 4 and step_scale = 3 are among the cases; so are float64 evaluations."""
    prm, init, rows, rep = S.oracle_case(dim, name)
    for j, (r, row) in enumerate(zip(rep, rows)):
        assert r["pose"] == tuple(row["pose"]), (j, r["pose"], row["pose"])
        assert r["done"] == (j == len(rows) - 1)
    S.check_rows(rep, rows, prm, name)


@pytest.mark.parametrize("dim", [2, 3])
def test_replay_of_a_float64_trace_is_exact_too(dim):
    if dim == 2:
        d, prm = S.pair2d(), S.params2d(hessian_mode=1, line_search=4, step_scale=3.0)
        rows = S.oracle_rows2d(o2.build_grid(d["tx"], d["ty"], prm), d["sx"], d["sy"], d["init"], prm, mirror32=False)
        rep = S.replay2d(d["init"], rows, prm)
    else:
        d, prm = S.pair3d(), S.params3d(hessian_mode=1, line_search=4, step_scale=3.0, max_iterations=20)
        rows = S.oracle_rows3d(o3.build_grid3(d["tx"], d["ty"], d["tz"], prm), d["sx"], d["sy"], d["sz"], d["init"], prm,
                               mirror32=False)
        rep = S.replay3d(d["init"], rows, prm)
    assert [r["pose"] for r in rep] == [tuple(row["pose"]) for row in rows]


def test_a_wrong_step_does_not_pass():
    """check_rows is not vacuous: a pose one part in 1e12 of the step off, a status and an iteration count off by one
    each fail it."""
    prm, init, rows, rep = S.oracle_case(2, "newton_far")
    for key, bad in (("pose", lambda p: (p[0] + 1e-12 * abs(rep[0]["applied"][0]) + 1e-15, p[1], p[2])),
                     ("status", lambda s: s + 1), ("iterations", lambda n: n + 1)):
        broken = [dict(r) for r in rows]
        broken[0][key] = bad(broken[0][key])
        with pytest.raises(AssertionError):
            S.check_rows(S.replay2d(init, broken, prm), broken, prm)


def test_oracle_error_is_an_eighth_of_the_tolerance():
    """The measurement behind C_STEP: the oracle's worst error of an applied step, against the exact solution of the
    damped system, over every step row of every case (and the one-point source), in units of eps * kappa * max|step|."""
    worst, n = (0.0, None), 0
    runs = [(d, name, S.oracle_case(d, name)) for d, name in ALL] + \
        [(2, "one_point", _one_point_rows()), (2, "origin_point", _one_point_rows(S.origin_point_pair))]
    for dim, name, (prm, init, rows, rep) in runs:
        for j, r in enumerate(rep):
            if r["kind"] != "step":
                continue
            ratio, err = S.oracle_error_ratio(r["H"], r["g"], r["rung"], r["applied"], prm, dim)
            assert err <= S.step_tolerance(r["H"], r["g"], r["rung"], r["applied"]) / 8.0, (dim, name, j, ratio, err)
            worst = max(worst, (ratio, (dim, name, j, r["rung"])))
            n += 1
    print(f"oracle error ratio: worst {worst[0]:.3f} at {worst[1]} over {n} step rows; C_STEP = {S.C_STEP}")
    assert n > 400
    # the documented figures are the measured ones: the ratio to two digits, C_STEP = 8 x ratio rounded up
    assert worst[0] <= S.MEASURED_ORACLE_RATIO < worst[0] + 0.01
    assert S.C_STEP == math.ceil(8.0 * S.MEASURED_ORACLE_RATIO)


@pytest.mark.parametrize("dim,name", ALL, ids=IDS)
def test_case_reaches_its_branch_on_the_oracle(dim, name):
    prm, init, rows, rep = S.oracle_case(dim, name)
    want = set((S.CASES2D if dim == 2 else S.CASES3D)[name][3])
    got = S.reached(rep, rows, prm)
    assert want <= got, (want, got, [(r["kind"], r["rung"], r["limit"]) for r in rep])


@pytest.mark.parametrize("dim,name", ALL, ids=IDS)
def test_no_oracle_stop_decision_is_marginal(dim, name):
    """The GPU file accepts either stop when a deciding norm lies within STOP_MARGIN of its threshold; the cases stay
    1e6 times clear of that margin, so the allowance never applies to them."""
    prm, init, rows, rep = S.oracle_case(dim, name)
    for r in rep:
        if r["kind"] == "step":
            assert not S.near_stop_threshold(r, prm)
            for v, e in zip(r["norms"], (prm.eps_trans, prm.eps_rot)):
                assert abs(v - e) > 1e6 * S.STOP_MARGIN * e


def test_one_point_source_climbs_the_ladder():
    """One source point, min_hits = 1: a Gauss-Newton Hessian of rank 2, singular to rounding - rung 1, and a scaled
    condition number above 1e6 for the tolerance to carry."""
    prm, init, rows, rep = _one_point_rows()
    assert rows[0]["n_hit"] == 1 and rep[0]["kind"] == "step" and rep[0]["rung"] >= 1
    assert S.scaled_condition(rep[0]["H"], 0) > 1e12 and 1e5 < S.scaled_condition(rep[0]["H"], rep[0]["rung"]) < 1e8
    # ... and the point at the origin of the source frame, whose Hessian is singular exactly
    prm, init, rows, rep = _one_point_rows(S.origin_point_pair)
    assert rows[0]["n_hit"] == 1 and rep[0]["kind"] == "step" and rep[0]["rung"] >= 1
    assert not rep[0]["H"][2].any() and not rep[0]["H"][:, 2].any()


def test_one_step_cases_reach_their_branch_at_row_0():
    """The drivers without a trace replay one update: the branch must show at row 0 already."""
    for dim in (2, 3):
        _, _, _, rep = S.oracle_case(dim, "newton_far")
        assert rep[0]["rung"] >= 5
        _, _, _, rep = S.oracle_case(dim, "tight_limits")
        assert rep[0]["limit"] in ("trans", "rot")


def test_global_table_pairs_exceed_the_on_chip_capacity():
    d = S.pair2d()
    for opt, beyond in ((dict(), False), (S.GLOBAL2D, True)):
        _, _, _, W, H = o2.grid_geometry(d["tx"], d["ty"], S.params2d(**opt).cell_size)
        assert (W > 143 and H > 143 and W * H > S.GLOBAL2D_ONCHIP_CELLS) == beyond and W * H <= 512 * 512, (W, H)
    d3 = S.pair3d()
    P = np.stack([d3["tx"], d3["ty"], d3["tz"]], axis=1)
    for opt, beyond in ((dict(), False), (S.GLOBAL3D, True)):
        dims = o3.grid_geometry3(P, S.params3d(**opt).cell_size)[2]
        assert (np.prod(dims) > 1.2 * S.GLOBAL3D_ONCHIP_CELLS) == beyond, dims
        assert beyond or np.prod(dims) < 0.8 * S.GLOBAL3D_ONCHIP_CELLS
    # ... and still give the solver something to do
    for name in S.ONE_STEP:
        _, start, opt, _ = S.CASES2D[name]
        prm = S.params2d(fixed_iterations=1, **S.GLOBAL2D, **opt)
        rows = S.oracle_rows2d(o2.build_grid(d["tx"], d["ty"], prm), d["sx"], d["sy"], start(), prm)
        assert rows[0]["status"] == o2.NDT_OK and rows[0]["n_hit"] >= 8
