"""The committed 3D pair at steep roll and pitch: cases and the one judge the tilted tests share.  CPU only.

Every other pose of the suite keeps |roll|, |pitch| <= 0.05 rad, where cos = 1 and sin = 0 to within the tolerances: a
wrong sin roll * sin pitch term of R = Rz Ry Rx, or a roll axis formed without the pitch, passes there.  tilted_pair
re-expresses the golden pair's SOURCE in a frame turned by Q = R(true)' R(angles), so that the pose which puts it onto
the untouched target is (true translation, angles): the same scene, the same target grid, the same world points (to
float32 rounding of the source), and every derivative of the rotation taken where its sines are large.

Poses are compared as translation plus rot_gap = |R(a) - R(b)|_F / sqrt 2 (the rotation angle between them, for small
ones), never componentwise in the angles: at cos pitch = 0.12 roll and yaw trade against each other eight to one.

judge_eval holds an evaluation (H, g, score, n_hit) to the float32-mirror oracle by the bounds of
test_gpu_ndt3d.test_evaluate3d_parity; the per-point float32 arithmetic does not depend on the attitude, so they are
those bounds and no others."""
from __future__ import annotations

import functools
import math

import numpy as np

import step_replay as S
from oracle import ndt3d as o3

ATTITUDES = {
    "steep": (0.7, -0.5, 2.1),
    "inverted": (-2.4, 1.1, -0.9),
    "near_gimbal": (1.2, 1.45, 0.4),                 # cos pitch = 0.12
}
SINGULAR = (0.4, math.pi / 2.0, -0.3)                # pitch = pi / 2: the roll and yaw axes coincide, H has rank 5

FAR_OFFSET = np.array((0.3, -0.2, 0.05, 0.01, -0.01, 0.03))             # the far start is the true pose MINUS this
EVAL_OFFSET = np.array((0.01, -0.01, 0.005, 0.001, -0.001, 0.002))
MAP_OFFSET = np.array((0.1, -0.08, 0.02, 0.004, -0.003, 0.01))          # the map-to-map start is the true pose minus this
NEWTON_NEAR = 0.002 * np.array((1.0, -1.0, 0.5, 0.1, -0.1, 0.2))        # test_newton_hessian_3d's start rule

TIGHT = dict(step_max_trans=0.02, step_max_rot=0.002, max_iterations=40)
LINE_SEARCH = dict(line_search=4, step_scale=3.0, max_iterations=30)

# align_trace cases: options, the branches (step_replay.reached) the oracle's run reaches from the far start and the
# device's must too.  On "steep" no line-search trial is rejected: every tripled step raises the score there.
TRACE_CASES = {"default": ({}, ("converged",)), "tight": (TIGHT, ("rot", "both_rot")), "line_search": (LINE_SEARCH, ("trial",))}
TRACE_NOT_REACHED = {("steep", "line_search"): ("trial",)}


def trace_case(name, case):
    opt, want = TRACE_CASES[case]
    return opt, tuple(b for b in want if b not in TRACE_NOT_REACHED.get((name, case), ()))


# judge_eval's bounds (test_evaluate3d_parity)
N_HIT_TOL = 3
H_TOL = 2e-4            # |dH_ij| / sqrt(H_ii H_jj)
SCORE_TOL = 2e-4        # |dscore| / score
G_TOL = 1e-3            # |dg_i| / sqrt(H_ii score)
POSE_TOL = 1e-4         # converged poses: metres, and rot_gap


def rot(angles) -> np.ndarray:
    return o3.rot_and_derivs(*angles)[0]


def rot_gap(a, b) -> float:
    """|R(a) - R(b)|_F / sqrt 2 of two (roll, pitch, yaw) triples or 6-poses: 2 sin(angle / 2) of the rotation between."""
    a, b = (tuple(v)[-3:] for v in (a, b))
    return float(np.linalg.norm(rot(a) - rot(b))) / math.sqrt(2.0)


def pose_gap(a, b):
    """(largest translation difference, rot_gap) of two 6-poses."""
    return float(np.abs(np.array(a[:3], dtype=np.float64) - np.array(b[:3], dtype=np.float64)).max()), rot_gap(a, b)


def wrapped(pose):
    return tuple(float(v) for v in pose[:3]) + tuple(S.o2.wrap_angle(float(v)) for v in pose[3:])


def tilt(d, angles):
    """A pair {"sx", "sy", "sz", "pose", ...} with its source re-expressed so that the true rotation is Rz Ry Rx(angles)."""
    Q = rot(d["pose"][3:]).T @ rot(angles)
    P = np.stack([d["sx"], d["sy"], d["sz"]], axis=1).astype(np.float64) @ Q                  # rows: s' = Q' s
    out = dict(d)
    out["sx"], out["sy"], out["sz"] = (np.ascontiguousarray(P[:, c].astype(np.float32)) for c in range(3))
    out["pose"] = tuple(float(v) for v in d["pose"][:3]) + tuple(float(v) for v in angles)
    out["init"] = tuple(np.array(out["pose"]) - FAR_OFFSET)
    return out


@functools.lru_cache(maxsize=None)
def _tilted(angles):
    return tilt(S.pair3d(), angles)


def tilted_pair(angles):
    """The golden pair with the source turned so that the true rotation is Rz Ry Rx(angles); `angles` a name of
    ATTITUDES or a triple.  "pose" is the true pose, "init" the far start.  The arrays are shared: do not write to them."""
    return _tilted(tuple(float(v) for v in (ATTITUDES[angles] if isinstance(angles, str) else angles)))


def far_start(name):
    return tilted_pair(name)["init"]


def eval_poses(name):
    p = np.array(tilted_pair(name)["pose"])
    return [tuple(p), tuple(p + EVAL_OFFSET)]


def map_start(name):
    return tuple(np.array(tilted_pair(name)["pose"]) - MAP_OFFSET)


@functools.lru_cache(maxsize=None)
def grid(cell_size: float = 1.0):
    """The target grid: one per cell size for every attitude, the target is untouched."""
    d = S.pair3d()
    return o3.build_grid3(d["tx"], d["ty"], d["tz"], o3.Ndt3Params(cell_size=cell_size))


def oracle_eval(d, pose, mode: int = 0, mirror32: bool = True, cell_size: float = 1.0):
    prm = o3.Ndt3Params(hessian_mode=mode, cell_size=cell_size)
    return o3.evaluate3(grid(cell_size), d["sx"], d["sy"], d["sz"], tuple(pose), prm, mirror32=mirror32)


@functools.lru_cache(maxsize=None)
def reference_run(name, mode: int = 0, start: str = "far", opts: tuple = (), mirror32: bool = False, cell_size: float = 1.0):
    """oracle.align3 on a tilted pair.  start: "far", or "near" = the float64 Gauss-Newton optimum from the far start
    plus NEWTON_NEAR.  opts: a tuple of (option, value).  Returns (start pose, result)."""
    d = tilted_pair(name)
    if start == "far":
        init = d["init"]
    else:
        init = tuple(np.array(reference_run(name, cell_size=cell_size)[1]["pose"]) + NEWTON_NEAR)
    prm = o3.Ndt3Params(hessian_mode=mode, cell_size=cell_size, **dict(opts))
    return init, o3.align3(grid(cell_size), d["sx"], d["sy"], d["sz"], wrapped(init), prm, mirror32=mirror32)


def eval_figures(got, ref, Hgn=None):
    """(|n_hit difference|, Jacobi-scaled |dH|, |dscore| / score, |dg| / sqrt(H_ii score)) of `got` against `ref`, both
    (H, g, score, n_hit).  The scale is ref's own diagonal; for a Newton H (which may be indefinite) pass the
    Gauss-Newton H of the same pose as Hgn, as test_newton_hessian_3d does."""
    H, g, s, n = got
    Hr, gr, sr, nr = ref
    dg = np.diag(Hr if Hgn is None else Hgn)
    sc = np.sqrt(np.outer(dg, dg))
    return (abs(int(n) - int(nr)), float(np.max(np.abs(np.asarray(H) - Hr) / sc)), abs(float(s) - sr) / sr,
            float(np.max(np.abs(np.asarray(g) - gr) / np.sqrt(dg * sr))))


def judge_eval(got, ref_mirror32, Hgn=None, label=""):
    """Assert the bounds of test_evaluate3d_parity on `got` against the float32-mirror oracle; returns the figures."""
    f = eval_figures(got, ref_mirror32, Hgn)
    assert f[0] <= N_HIT_TOL and f[1] < H_TOL and f[2] < SCORE_TOL and f[3] < G_TOL, \
        (label, dict(zip(("n_hit", "H", "score", "g"), f)))
    return f


NEWTON_FLOOR = 2e-5     # the project's bound on H against the mirror oracle (d2d3_ref.EVAL_FLOOR)


def newton_block(Hn, Hg, Hgn_ref):
    """The rotation block of (Newton H - Gauss-Newton H) of one pose, Jacobi-scaled by the oracle's Gauss-Newton diagonal:
    - d2 sum w (J'v)(J'v)' plus the second derivatives of R against M = sum w v p' (newton_rot_block3).  The per-point
    Gauss-Newton terms, which carry most of an evaluation's float32 noise, cancel in it; judge_eval's 2e-4 is ten times
    wider than a lost u w' term of d2R/dpitch2 is worth (tests/test_tilted_ref.py), this is not."""
    d = np.sqrt(np.diag(Hgn_ref)[3:])
    return (np.asarray(Hn)[3:, 3:] - np.asarray(Hg)[3:, 3:]) / np.outer(d, d)


def newton_block_bound(d, poses):
    """d2d3_ref.eval_bounds' rule on the oracle itself: 4 x its largest float32-mirror-vs-float64 difference of the
    block over `poses`, floored at NEWTON_FLOOR.  Returns (bound, measured)."""
    worst = 0.0
    for pose in poses:
        e = [(oracle_eval(d, pose, 1, m)[0], oracle_eval(d, pose, 0, m)[0]) for m in (True, False)]
        worst = max(worst, float(np.abs(newton_block(*e[0], e[1][1]) - newton_block(*e[1], e[1][1])).max()))
    return max(4.0 * worst, NEWTON_FLOOR), worst


class Worst:
    """The largest figure of each quantity per key, for the numbers the docstrings carry."""

    def __init__(self):
        self.rows = {}

    def add(self, key, figures):
        old = self.rows.get(key)
        self.rows[key] = tuple(figures) if old is None else tuple(max(a, b) for a, b in zip(old, figures))

    def report(self, title, names=("n_hit", "H", "score", "g")):
        print(f"\n{title}")
        for key, f in self.rows.items():
            print(f"    {key}: " + ", ".join(f"{n} {v:.3g}" for n, v in zip(names, f)))


# The map-to-map score volume at a steep pinned roll and pitch (tests/test_gpu_search_map3d.py): that file's small pair
# (synth3d.make_pair3d, 32 x 1024 beams, this generating pose) with the source tilted to "steep", 1 m voxels, and a
# window of 5 x 9 x 9 = 405 poses - no larger than that file's smallest - round the pose that puts it back.
MAP_SEARCH_POSE = (2.0, -1.5, 0.02, 0.004, -0.003, 0.6)
MAP_SEARCH_LATTICE = (5, 9, 9)


@functools.lru_cache(maxsize=None)
def map_search_pair():
    from gtsam_ndt_amd import synth3d
    return tilt(synth3d.make_pair3d(n_elev=32, n_azim=1024, pose=MAP_SEARCH_POSE), ATTITUDES["steep"])


def map_search_window():
    from gtsam_ndt_amd import search
    p, a = MAP_SEARCH_POSE, ATTITUDES["steep"]
    return search.Window((p[0] + 0.1, p[1] + 0.1, p[2] + 0.05, a[0], a[1], a[2] + 0.02), (0.5, 0.5, 0.1), (0.125, 0.125, 0.05))
