"""Replay of single solve / update steps (docs/ALGORITHM.md sections 2.5 and 2.6) against the float64 oracle.  CPU only,
but for one_step_results at the end: the list of alignment drivers the GPU files share.

A result row carries, as doubles, exactly what the device fed its solver: H, g, score, n_hit.  rows[j] holds the pose
after update j + 1 and the sums of the evaluation behind it, taken at rows[j - 1].pose (include/ndt_hip.h, the trace
contract), so oracle.gn_update(rows[j - 1].pose, rows[j].H, rows[j].g, ...) must reproduce rows[j].pose, iterations and
status to the accuracy of a float64 solve: the float32 evaluation noise cancels, both sides start from the same doubles.

replay2d / replay3d walk such rows, step_tolerance is the bound a step is held to, exact_step the rational-arithmetic
truth that bound is calibrated against, and CASES2D / CASES3D are the inputs the CPU file (tests/test_step_replay.py:
the oracle reaches every branch on them) and the GPU file (tests/test_gpu_step_replay.py) share.

The constant of step_tolerance.  The error of a backward-stable solve of A x = b is a small multiple of eps * kappa * |x|,
kappa the condition number of the Jacobi-scaled matrix (van der Sluis: within a factor n of the best diagonal scaling).
The multiple is measured, not guessed: test_step_replay.test_oracle_error_is_an_eighth_of_the_tolerance solves every
damped system of every row of every CPU case exactly (fractions.Fraction: the doubles of H and g are rationals), applies
step_scale and the limits in 80-digit decimals, and takes the oracle's worst error of an applied step entry in units of
eps * kappa * max|step|:

    measured ratio  MEASURED_ORACLE_RATIO = 1.53   (1.520 on row 28 of the 3D line-search case, rung 0, kappa 233; the
                                                    worst of 461 step rows, ladder rungs 0 to 8, kappa 1.1 to 2e6)
    C_STEP = 8 * ratio, rounded up = 13

The device runs the same elimination with reciprocal-multiply (v_rcp_f64 + two Newton steps) and FMA contraction in
place of the divisions, a handful of extra roundings per pivot, hence the factor 8 and no more.
"""
from __future__ import annotations

import dataclasses
import decimal
import functools
import math
import os
from fractions import Fraction

import numpy as np

from oracle import ndt2d as o2
from oracle import ndt3d as o3

EPS = 2.0 ** -52
MEASURED_ORACLE_RATIO = 1.53
C_STEP = 13.0
STOP_MARGIN = 1e-9            # a deciding norm this close (relative) to eps_trans / eps_rot may stop either way

# lam of rung k, computed as the solvers compute it
LADDER = [0.0, 1e-6]
while len(LADDER) < o2.LM_ATTEMPTS:
    LADDER.append(LADDER[-1] * 10.0)

_D = decimal.Decimal
_CTX = decimal.Context(prec=80)


def _get(row, key):
    return row[key] if isinstance(row, dict) else getattr(row, key)


def damped(H, rung: int) -> np.ndarray:
    """H + lam * diag(max(|H_ii|, 1e-12)) at the rung's lam."""
    H = np.asarray(H, dtype=np.float64)
    return H + LADDER[rung] * np.diag(np.maximum(np.abs(np.diag(H)), 1e-12))


def rung_of(H, g, d) -> int:
    """The ladder rung a solution d of (H + lam diag|H|) d = -g was solved at: the one whose system d satisfies best.
    Neighbouring rungs differ by at least 1e-6 |H_ii| |d_i| in the residual, far above the solve's own residual."""
    g, d = np.asarray(g, dtype=np.float64), np.asarray(d, dtype=np.float64)
    res = [np.abs(damped(H, k) @ d + g).max() for k in range(len(LADDER))]
    return int(np.argmin(res))


def scaled_condition(H, rung: int) -> float:
    """2-norm condition number of D^-1/2 (H + lam diag|H|) D^-1/2, D the diagonal of the damped matrix."""
    A = damped(H, rung)
    s = 1.0 / np.sqrt(np.maximum(np.abs(np.diag(A)), 1e-300))
    return float(np.linalg.cond(A * np.outer(s, s), 2))


def step_tolerance(H, g, rung: int, applied_step, pose=None, c: float = C_STEP):
    """c * eps * kappa * max|applied step| - the step after step_scale and the limits - plus, with `pose`, a floor of
    4 ulp of each pose entry (the addition, the angle wrap).  g is part of the signature because the tolerance belongs to
    the system (H, g); the bound itself does not depend on it."""
    size = float(np.abs(np.asarray(applied_step, dtype=np.float64)).max())
    tol = c * EPS * scaled_condition(H, rung) * size if size > 0.0 else 0.0       # (H = 0, g = 0: no step, any kappa)
    if pose is None:
        return tol
    return tol + 4.0 * np.spacing(np.abs(np.asarray(pose, dtype=np.float64)))


def _limits(d, nt_count: int, prm):
    """The oracle's scale-and-limit rule on a solved step: (applied step, which limit scaled it, the two norms the stop
    rule tests)."""
    d = np.asarray(d, dtype=np.float64) * prm.step_scale
    nt = math.sqrt(sum(float(v) ** 2 for v in d[:nt_count]))
    nr = abs(float(d[2])) if nt_count == 2 else math.sqrt(sum(float(v) ** 2 for v in d[3:]))
    alpha, limit = 1.0, "none"
    if nt > prm.step_max_trans:
        alpha, limit = prm.step_max_trans / nt, "trans"
    if nr * alpha > prm.step_max_rot:
        alpha, limit = prm.step_max_rot / nr, "rot"
    return d * alpha, limit, (nt * alpha, nr * alpha)


def exact_step(H, g, rung: int, prm, nt_count: int):
    """The applied step of the damped system solved exactly: Gaussian elimination over the rationals, then step_scale
    and the limits in 80-digit decimals.  Returns decimals."""
    n = len(g)
    H = np.asarray(H, dtype=np.float64)
    lam = Fraction(LADDER[rung])
    A = [[Fraction(float(H[i, j])) for j in range(n)] + [-Fraction(float(g[i]))] for i in range(n)]
    for i in range(n):
        A[i][i] += lam * Fraction(max(abs(float(H[i, i])), 1e-12))
    for j in range(n):
        p = max(range(j, n), key=lambda r: abs(A[r][j]))
        A[j], A[p] = A[p], A[j]
        for r in range(n):
            if r != j and A[r][j] != 0:
                f = A[r][j] / A[j][j]
                A[r] = [a - f * b for a, b in zip(A[r], A[j])]
    scale = Fraction(float(prm.step_scale))
    x = [A[i][n] / A[i][i] * scale for i in range(n)]
    dx = [_CTX.divide(_D(v.numerator), _D(v.denominator)) for v in x]
    sq = lambda vs: _CTX.sqrt(sum((_CTX.multiply(v, v) for v in vs), _D(0)))
    nt = sq(dx[:nt_count])
    nr = abs(dx[2]) if nt_count == 2 else sq(dx[3:])
    alpha = _D(1)
    if nt > _D(float(prm.step_max_trans)):
        alpha = _CTX.divide(_D(float(prm.step_max_trans)), nt)
    if _CTX.multiply(nr, alpha) > _D(float(prm.step_max_rot)):
        alpha = _CTX.divide(_D(float(prm.step_max_rot)), nr)
    return [_CTX.multiply(v, alpha) for v in dx]


def oracle_error_ratio(H, g, rung: int, applied_step, prm, nt_count: int):
    """The worst entry of |applied_step - exact_step|: in units of eps * kappa * max|exact step|, and as it is."""
    ex = exact_step(H, g, rung, prm, nt_count)
    err = max(abs(_CTX.subtract(_D(float(a)), e)) for a, e in zip(applied_step, ex))
    unit = EPS * scaled_condition(H, rung) * float(max(abs(e) for e in ex))
    return float(err) / unit, float(err)


def _replay(nt_count: int, init_pose, rows, prm, update, solve):
    wrap = o2.wrap_angle
    pose = tuple(float(v) for v in init_pose[:nt_count]) + tuple(wrap(float(v)) for v in init_pose[nt_count:])
    ls = {} if prm.line_search > 0 else None
    it = 0
    out = []
    for row in rows:
        H = np.asarray(_get(row, "H"), dtype=np.float64)
        g = np.asarray(_get(row, "g"), dtype=np.float64)
        n_hit, score = int(_get(row, "n_hit")), float(_get(row, "score"))
        trials_before = ls.get("trials", 0) if ls else 0
        was_valid = bool(ls and ls.get("valid"))
        new_pose, it, status, done = update(pose, H, g, n_hit, it, prm, score, ls)
        r = {"start": pose, "pose": tuple(float(v) for v in new_pose), "iterations": it, "status": status, "done": done,
             "kind": "stop", "rung": None, "limit": "none", "applied": None, "norms": None, "solved": None, "H": H,
             "g": g}
        if was_valid and ls["trials"] == trials_before + 1:
            # a rejected line-search trial: the pose is base + alpha * step of the solve the state came from
            r.update(kind="trial", rung=ls["rung"], H=ls["H"], g=ls["g"], applied=ls["alpha"] * np.array(ls["step"]))
        elif n_hit >= prm.min_hits and status != o2.NDT_DEGENERATE_HESSIAN:
            d, ok = solve(H, g)
            assert ok
            applied, limit, norms = _limits(d, nt_count, prm)
            r.update(kind="step", rung=rung_of(H, g, d), limit=limit, applied=applied, norms=norms, solved=np.array(d))
            if ls is not None:
                ls.update(rung=r["rung"], H=H, g=g)
        out.append(r)
        pose = tuple(float(v) for v in _get(row, "pose"))      # the next row's evaluation was taken at THIS row's pose
    return out


def replay2d(init_pose, rows, prm):
    """One dict per row: the oracle's pose / iterations / status / done from the row before's pose (the wrapped initial
    pose for row 0) and the row's H, g, n_hit, score, with the line-search state carried along; kind ("step", "trial": a
    rejected line-search trial, "stop": no update), the ladder rung, the limit that scaled the step ("trans", "rot",
    "none"), the solved step, the applied step and the (translation, rotation) norms of the stop rule; H, g = the system
    the step came from (a trial's is its base step's)."""
    return _replay(2, init_pose, rows, prm, o2.gn_update, o2.solve3)


def replay3d(init_pose, rows, prm):
    return _replay(3, init_pose, rows, prm, o3.gn_update3, o3.solve_ldl)


def near_stop_threshold(r, prm) -> bool:
    """Whether a deciding norm of a step row lies within STOP_MARGIN (relative) of its threshold."""
    if r["kind"] != "step" or prm.fixed_iterations > 0:
        return False
    return any(abs(v - e) <= STOP_MARGIN * e for v, e in zip(r["norms"], (prm.eps_trans, prm.eps_rot)))


def crossed_pi(r, angle_index: int) -> bool:
    """The step moved this angle over +-pi (and wrap_angle brought it back)."""
    if r["kind"] != "step":
        return False
    return abs(r["start"][angle_index] + r["applied"][angle_index]) > math.pi and abs(r["pose"][angle_index]) <= math.pi


def check_rows(replayed, rows, prm, label=""):
    """What every replayed row is held to: pose within step_tolerance (angles wrapped to (-pi, pi] and compared on the
    circle: pi and -pi + 1 ulp are neighbours), iterations and status equal, done on the last row and only there (either
    stop accepted within STOP_MARGIN of a threshold)."""
    assert len(replayed) == len(rows) and rows, label
    for j, (r, row) in enumerate(zip(replayed, rows)):
        pose = np.array(_get(row, "pose"), dtype=np.float64)
        nt = 2 if len(pose) == 3 else 3
        where = (label, j, r["kind"], r["rung"], r["limit"])
        assert np.all(pose[nt:] > -math.pi) and np.all(pose[nt:] <= math.pi), (where, pose)
        tol = np.zeros(len(pose)) if r["kind"] == "stop" else \
            step_tolerance(r["H"], r["g"], r["rung"], r["applied"], pose=pose)
        diff = np.abs(pose - np.array(r["pose"]))
        diff[nt:] = np.minimum(diff[nt:], np.abs(2.0 * math.pi - diff[nt:]))
        assert np.all(diff <= tol), (where, diff, tol)
        if near_stop_threshold(r, prm):
            continue
        assert _get(row, "iterations") == r["iterations"] and _get(row, "status") == r["status"], \
            (where, _get(row, "iterations"), r["iterations"], _get(row, "status"), r["status"])
        assert r["done"] == (j == len(rows) - 1), (where, r["done"], len(rows))


# ------------------------------------------------------------------------------------------------ oracle traces as rows
def _rows_from_trace(trace, result, replay, init_pose, prm):
    """The oracle's trace (entry j: pose BEFORE update j + 1 and its evaluation) in the layout of device rows (pose AFTER
    the update), iterations and status filled in from the loop itself."""
    rows = []
    for j, t in enumerate(trace):
        after = trace[j + 1]["pose"] if j + 1 < len(trace) else result["pose"]
        rows.append({"pose": tuple(after), "H": t["H"], "g": t["g"], "score": t["score"], "n_hit": t["n_hit"]})
    for r, row in zip(replay(init_pose, rows, prm), rows):
        row["iterations"], row["status"] = r["iterations"], r["status"]
    assert rows[-1]["iterations"] == result["iterations"] and rows[-1]["status"] == result["status"]
    return rows


def oracle_rows2d(grid, sx, sy, init_pose, prm, mirror32=True):
    init = (init_pose[0], init_pose[1], o2.wrap_angle(init_pose[2]))
    trace = []
    res = o2.align(grid, sx, sy, init, prm, mirror32=mirror32, trace=trace)
    return _rows_from_trace(trace, res, replay2d, init, prm)


def oracle_rows3d(grid, sx, sy, sz, init_pose, prm, mirror32=True):
    init = tuple(init_pose[:3]) + tuple(o2.wrap_angle(v) for v in init_pose[3:])
    trace = []
    res = o3.align3(grid, sx, sy, sz, init, prm, mirror32=mirror32, trace=trace)
    return _rows_from_trace(trace, res, replay3d, init, prm)


# ------------------------------------------------------------------------------------------------------------- the cases
GOLD3 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ndt3d_small.npz")
PI = math.pi


@functools.lru_cache(maxsize=None)
def pair2d():
    """synth.make_pair(1): 1000 / 1000 points, the smallest 2D pair the project has."""
    from gtsam_ndt_amd import synth
    return synth.make_pair(1)


@functools.lru_cache(maxsize=None)
def pair3d():
    """The committed 4096-point 3D pair."""
    z = np.load(GOLD3)
    return {k: z[k] for k in ("tx", "ty", "tz", "sx", "sy", "sz")} | {"init": tuple(z["init"]), "pose": tuple(z["true_pose"])}


def _rot2(x, y, phi):
    c, s = math.cos(phi), math.sin(phi)
    return (c * x - s * y).astype(np.float32), (s * x + c * y).astype(np.float32)


@functools.lru_cache(maxsize=None)
def wrap_pair2d():
    """pair2d with the target turned about the origin so that the true heading is pi - 0.005."""
    d = dict(pair2d())
    phi = PI - 0.005 - d["pose"][2]
    d["tx"], d["ty"] = _rot2(d["tx"].astype(np.float64), d["ty"].astype(np.float64), phi)
    return d


@functools.lru_cache(maxsize=None)
def wrap_pair3d():
    """pair3d with the target turned about z so that the true yaw is pi - 0.005, and the source turned about its own x
    axis so that the true roll is -pi + 0.004: R_true Rx(psi) = Rz Ry Rx(roll + psi)."""
    d = dict(pair3d())
    phi = PI - 0.005 - d["pose"][5]
    d["tx"], d["ty"] = _rot2(d["tx"].astype(np.float64), d["ty"].astype(np.float64), phi)
    psi = -PI + 0.004 - d["pose"][3]
    y, z = d["sy"].astype(np.float64), d["sz"].astype(np.float64)       # s' = Rx(-psi) s
    c, s = math.cos(-psi), math.sin(-psi)
    d["sy"], d["sz"] = (c * y - s * z).astype(np.float32), (s * y + c * z).astype(np.float32)
    return d


def _true2(off):
    return tuple(np.array(pair2d()["pose"]) + np.array(off))


# name -> (pair, start pose, options, the branches the oracle must reach on it)
CASES2D = {
    "gn_default": (pair2d, lambda: pair2d()["init"], {}, ("rung0", "converged")),
    "newton_far": (pair2d, lambda: _true2((0.3, -0.2, 0.05)), dict(hessian_mode=1), ("row0_rung5",)),
    "tight_limits": (pair2d, lambda: _true2((-0.35, 0.15, -0.03)), dict(step_max_trans=0.02, step_max_rot=0.002),
                     ("trans", "rot", "both_trans", "both_rot")),
    "wrap": (wrap_pair2d, lambda: (0.0, 0.0, -PI + 0.02), {}, ("crossed2",)),
    "over_relaxed": (pair2d, lambda: pair2d()["init"], dict(step_scale=3.0, step_max_trans=0.05),
                     ("scale_limited", "converged")),
    "line_search": (pair2d, lambda: _true2((-0.3, 0.2, 0.0)), dict(line_search=4, step_scale=3.0),
                    ("trial", "trials_spent", "scale_kept_going")),
    "cut_off": (pair2d, lambda: pair2d()["init"], dict(max_iterations=4), ("not_converged4",)),
    "fixed": (pair2d, lambda: pair2d()["init"], dict(fixed_iterations=5), ("fixed5",)),
}
CASES3D = {
    "gn_default": (pair3d, lambda: pair3d()["init"], {}, ("rung0", "converged")),
    "newton_far": (pair3d, lambda: pair3d()["init"], dict(hessian_mode=1, max_iterations=30), ("row0_rung5",)),
    "tight_limits": (pair3d, lambda: tuple(np.array(pair3d()["pose"]) - np.array((0.5, -0.4, 0.1, 0.0, 0.0, 0.0))),
                     dict(step_max_trans=0.02, step_max_rot=0.002, max_iterations=40),
                     ("trans", "rot", "both_trans", "both_rot")),
    "wrap": (wrap_pair3d, lambda: (0.0, 0.0, 0.0, PI - 0.006, 0.0, -PI + 0.02), {}, ("crossed3", "crossed5")),
    "over_relaxed": (pair3d, lambda: pair3d()["init"], dict(step_scale=3.0, step_max_trans=0.08, max_iterations=30),
                     ("scale_limited",)),
    "line_search": (pair3d, lambda: pair3d()["init"], dict(line_search=4, step_scale=3.0, max_iterations=30), ("trial",)),
    "cut_off": (pair3d, lambda: pair3d()["init"], dict(max_iterations=4), ("not_converged4",)),
    "fixed": (pair3d, lambda: pair3d()["init"], dict(fixed_iterations=5), ("fixed5",)),
}


def params2d(**kw):
    """oracle parameters from the device's option names."""
    kw = dict(kw)
    if "overlap_grids" in kw:
        kw["overlap"] = kw.pop("overlap_grids")
    return o2.NdtParams(**kw)


def params3d(**kw):
    return o3.Ndt3Params(**kw)


def _unscaled(prm):
    return dataclasses.replace(prm, step_scale=1.0)


def reached(replayed, rows, prm) -> set:
    """The branch names (the last field of a case) a replay went through."""
    got = set()
    steps = [r for r in replayed if r["kind"] == "step"]
    if steps and all(r["rung"] == 0 for r in steps):
        got.add("rung0")
    if replayed[0]["kind"] == "step" and replayed[0]["rung"] >= 5:
        got.add("row0_rung5")
    if steps and max(r["rung"] for r in steps) >= 1:
        got.add("rung1")
    got |= {r["limit"] for r in steps} - {"none"}
    for a in (2, 3, 4, 5):
        if any(crossed_pi(r, a) for r in steps if a < len(r["pose"])):
            got.add(f"crossed{a}")
    if any(r["kind"] == "trial" for r in replayed):
        got.add("trial")
    if any(a["kind"] == "trial" and b["kind"] == "step" and prm.line_search > 0 and
           sum(1 for r in replayed[max(0, j - prm.line_search + 1):j + 1] if r["kind"] == "trial") == prm.line_search
           for j, (a, b) in enumerate(zip(replayed, replayed[1:]))):
        got.add("trials_spent")             # line_search halvings in a row, then a step from where they ended
    nt = 2 if len(replayed[0]["pose"]) == 3 else 3
    for r in steps:
        # both norms over their limits: the rotation test must see the step the translation limit already shortened
        full = _limits(r["solved"], nt, dataclasses.replace(prm, step_max_trans=math.inf, step_max_rot=math.inf))[2]
        if full[0] > prm.step_max_trans and full[1] > prm.step_max_rot:
            got.add("both_" + r["limit"])
        # the limits and the stop rule see the scaled step: the unscaled one would have passed / stopped
        if r["limit"] != "none" and _limits(r["solved"], nt, _unscaled(prm))[1] == "none":
            got.add("scale_limited")
        if not r["done"] and all(v / prm.step_scale < e for v, e in zip(r["norms"], (prm.eps_trans, prm.eps_rot))):
            got.add("scale_kept_going")
    last = replayed[-1]
    if last["done"] and last["status"] == o2.NDT_OK and prm.fixed_iterations == 0 and last["kind"] == "step":
        got.add("converged")
    if last["done"] and last["status"] == o2.NDT_NOT_CONVERGED and len(replayed) == 4 and last["iterations"] == 4:
        got.add("not_converged4")
    if last["done"] and last["status"] == o2.NDT_OK and len(replayed) == 5 and prm.fixed_iterations == 5:
        got.add("fixed5")
    return got


# The drivers without a trace are replayed over one update (fixed_iterations = 1: the row's H, g are those of the
# evaluation at the wrapped initial pose), with the options and starts of these two cases.
ONE_STEP = ("newton_far", "tight_limits")

# Pairs the batches must hand to their global-table variants: a grid beyond the on-chip capacity.  2D: 20480 cells
# (143 x 143; csrc/ndt2d_batch.hpp BatchLarge) - pair2d's 8 m room at 5.5 cm cells, min_points 2 so that a 1000-point
# cloud still fills cells.  3D: 6 bytes of the 160 KiB of LDS per voxel behind a 3216-byte head (csrc/ndt3d_batch.hpp,
# process_pair3's capacity test), i.e. 26770 voxels - pair3d at 0.75 m voxels.
GLOBAL2D = dict(cell_size=0.055, min_points=2)
GLOBAL2D_ONCHIP_CELLS = 20480
GLOBAL3D = dict(cell_size=0.75)
GLOBAL3D_ONCHIP_CELLS = (160 * 1024 - 3216) // 6


def one_point_pair(i: int = 0):
    """pair2d's target and point i of its source: with min_hits = 1 a Gauss-Newton Hessian of rank 2.  From float64
    per-point terms (the oracle's) it is singular to 1e-13 of its scale and the solve climbs to rung 1; the device's terms
    are float32, its H is singular to 1e-8 only, and whether the last pivot passes at rung 0 is a matter of rounding."""
    d = pair2d()
    return d["sx"][i:i + 1].copy(), d["sy"][i:i + 1].copy(), d["init"], dict(min_hits=1)


def origin_point_pair():
    """A source point at the origin of its frame, put onto the first target point: the rotation does not move it, the
    Hessian's rotation row and column are exactly zero in any arithmetic, and rung 0 fails for certain (pivot 0, damped
    to 1e-6 * 1e-12 at rung 1)."""
    d = pair2d()
    z = np.zeros(1, dtype=np.float32)
    return z, z.copy(), (float(d["tx"][0]), float(d["ty"][0]), 0.3), dict(min_hits=1)


@functools.lru_cache(maxsize=None)
def oracle_case(dim: int, name: str):
    """(prm, start, rows, replayed) of a case on the float32-mirror oracle."""
    pair, start, opt, _ = (CASES2D if dim == 2 else CASES3D)[name]
    d, init = pair(), tuple(start())
    if dim == 2:
        prm = params2d(**opt)
        rows = oracle_rows2d(o2.build_grid(d["tx"], d["ty"], prm), d["sx"], d["sy"], init, prm)
        return prm, init, rows, replay2d(init, rows, prm)
    prm = params3d(**opt)
    rows = oracle_rows3d(o3.build_grid3(d["tx"], d["ty"], d["tz"], prm), d["sx"], d["sy"], d["sz"], init, prm)
    return prm, init, rows, replay3d(init, rows, prm)


# ----------------------------------------------------------------------------- one update of every driver (needs a GPU)
SPLIT_FROM = 12              # NDT_TUNE_SPLIT_FROM's default: calls of at least this many starts run the two-kernel chain


def device_api(dim):
    from gtsam_ndt_amd import matcher as M
    if dim == 2:
        return M.NdtMatcher2D, M.NdtBatch2D, params2d, replay2d, ("tx", "ty"), ("sx", "sy")
    return M.NdtMatcher3D, M.NdtBatch3D, params3d, replay3d, ("tx", "ty", "tz"), ("sx", "sy", "sz")


def _cuda(arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _starts(init, m):
    """m starts a millimetre apart: each result is replayed from its own."""
    step = np.array((1e-3, -1e-3, 1e-4) if len(init) == 3 else (1e-3, -1e-3, 5e-4, 1e-4, -1e-4, 1e-4))
    return [tuple(np.array(init) + k * step) for k in range(m)]


def one_step_results(dim, name, pair=None, init=None):
    """One update (fixed_iterations = 1) of every alignment driver with the options of case `name`, on the case's own
    pair and start or on the given ones (tests/test_gpu_tilted3d.py: the tilted pairs).  Yields
    (driver, result, the pose it started from, the options, whether it evaluates the case's own point-to-map objective)."""
    Matcher, Batch, params, replay, tk, sk = device_api(dim)
    case_pair, start, opt, _ = (CASES2D if dim == 2 else CASES3D)[name]
    d = case_pair() if pair is None else pair
    init = tuple(start()) if init is None else tuple(init)
    kw = dict(opt, fixed_iterations=1)
    kw.pop("max_iterations", None)
    tgt, src = [d[k] for k in tk], [d[k] for k in sk]
    singles = [("k_align_small", {}, {}), ("k_iterate", {"short_scan_kernel": 0}, {}),
               ("k_iterate, 1024 threads", {"short_scan_kernel": 0, "wide_threshold": 500}, {}),
               ("k_iterate, 4 overlapping grids", {"short_scan_kernel": 0}, {"overlap_grids": 4})] if dim == 2 else \
        [("k_iterate3", {}, {})]
    for label, tuning, extra in singles:
        with Matcher(tuning=tuning, **kw, **extra) as m:
            m.set_target(*tgt)
            yield label, m.align(*src, init), init, kw | extra, not extra
    with Matcher(**kw) as m:
        m.set_target(*tgt)
        dev = _cuda(src)
        for n in (2, SPLIT_FROM):
            starts = _starts(init, n)
            for k, r in enumerate(m.align_multi_start(*dev, starts)):
                yield f"align_multi_start, {n} starts [{k}]", r, starts[k], kw, True
            for k, r in enumerate(m.align_multi_scan([dev] * n, starts)):
                yield f"align_multi_scan, {n} scans [{k}]", r, starts[k], kw, True
    variants = [("batch, small variant", dict(small_variant=True), {}, 0), ("batch, 1024 threads", dict(small_variant=False), {}, 1),
                ("batch, global tables", dict(global_workgroups=8), GLOBAL2D, 1)] if dim == 2 else \
        [("batch3, on chip", {}, {}, None), ("batch3, global tables", dict(global_workgroups=8), GLOBAL3D, None)]
    for label, how, extra, large in variants:
        with Batch(**how, **kw, **extra) as b:
            r = b.align([tuple(tgt)], [tuple(src)], [init])[0]
            assert large is None or b.last_large_count == large, (label, b.last_large_count)
        yield label, r, init, kw | extra, not extra
    with Matcher(**kw) as t, Matcher(**kw) as s:
        t.set_target(*tgt)
        s.set_target(*src)
        yield "align_map", t.align_map(s, init), init, kw, False
