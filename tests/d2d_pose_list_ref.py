"""Restatement of the map-to-map score at a list of poses (docs/ALGORITHM.md section 2.21): what
ndt2d_score_map_poses* / ndt3d_score_map_poses* are held to.

TEST INFRASTRUCTURE ONLY (imported by tests/test_d2d_pose_list_ref.py and tests/test_gpu_score_map_poses*.py).
scores2d / scores3d are d2d_ref.evaluate / d2d3_ref.evaluate per finite pose - score and n_hit - and (0, 0) for a pose with
a non-finite coordinate.  mirror32=False is the float64 form the device is held to; mirror32=True rounds every
per-component operation to float32 and bounds the device's own rounding.

The lists and lattices the CPU and the GPU tests share are defined here, so that the bound the CPU test supports is the
bound of the very poses the GPU tests score."""
from __future__ import annotations

import math

import numpy as np

import d2d3_ref as R3
import d2d_ref as R2
from gtsam_ndt_amd import search, synth, synth3d
from oracle import ndt2d as O2
from oracle import ndt3d as O3

POSE3 = (2.0, -1.5, 0.02, 0.004, -0.003, 0.6)          # the generating pose of the 3D pairs (test_gpu_search_map3d.py)
SPREAD3 = (0.8, 0.8, 0.4, 0.1, 0.1, math.pi)
SPREAD2 = (0.8, 0.8, math.pi)
# the loop closure of two 3D submaps whose relative height and tilt are unknown
LOOP_POSE3 = (2.0, -1.5, 0.35, 0.07, -0.05, 0.6)
LOOP_BEST3 = (2.05, -1.54, 0.4, 0.06, -0.04, 0.605)    # the best pose of loop_list3(): checked on the CPU (float64)

_cache = {}


def scores2d(tgt, comps, poses, prm, mirror32: bool = False):
    """(score float64 [m], n_hit int64 [m]) at poses [m, 3]."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    sc, nh = np.zeros(poses.shape[0]), np.zeros(poses.shape[0], dtype=np.int64)
    for i, p in enumerate(poses):
        if np.all(np.isfinite(p)):
            _, _, sc[i], nh[i] = R2.evaluate(tgt, comps, tuple(float(v) for v in p), prm, mirror32)
    return sc, nh


def scores3d(tgt, comps, poses, prm, mirror32: bool = False):
    """(score float64 [m], n_hit int64 [m]) at poses [m, 6]."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 6)
    sc, nh = np.zeros(poses.shape[0]), np.zeros(poses.shape[0], dtype=np.int64)
    for i, p in enumerate(poses):
        if np.all(np.isfinite(p)):
            _, _, sc[i], nh[i] = R3.evaluate(tgt, comps, tuple(float(v) for v in p), prm, mirror32)
    return sc, nh


def lattice_list(window) -> np.ndarray:
    """The lattice of a search window as a list in flat index order, with the lattice's own doubles: [m, 3], or [m, 6]
    with rows (x, y, c[2], c[3], c[4], yaw) for a 3D window."""
    c = window[0]
    xs, ys, th = search.lattice(window)
    T, Y, X = np.meshgrid(th, ys, xs, indexing="ij")
    one = np.ones(X.size)
    mid = [c[a] * one for a in (2, 3, 4)] if len(c) == 6 else []
    return np.stack([X.ravel(), Y.ravel(), *mid, T.ravel()], axis=1)


def near_list(center, spread, seed: int, n: int = 128) -> np.ndarray:
    """n uniform poses within +-spread of `center`, and that pose itself."""
    rng = np.random.default_rng(seed)
    c = np.asarray(center, dtype=np.float64)
    return np.concatenate([c[None, :] + rng.uniform(-1.0, 1.0, (n, c.size)) * np.asarray(spread), c[None, :]])


# ---- the pairs (cached per process: the CPU test and the GPU tests run in one)
def pair3(size: str = "small", pose=POSE3):
    key = ("pair3", size, pose)
    if key not in _cache:
        ne, na = {"small": (32, 1024), "full": (64, 2048)}[size]
        _cache[key] = synth3d.make_pair3d(n_elev=ne, n_azim=na, pose=pose)
    return _cache[key]


def maps3(size: str = "small", cell: float = 1.0, pose=POSE3):
    """(target grid, source components, parameters) of the restatement for a 3D pair."""
    key = ("maps3", size, cell, pose)
    if key not in _cache:
        d = pair3(size, pose)
        prm = O3.Ndt3Params(cell_size=cell)
        tgt, _ = R3.build_map(d["tx"], d["ty"], d["tz"], prm)
        _, comps = R3.build_map(d["sx"], d["sy"], d["sz"], prm)
        _cache[key] = (tgt, comps, prm)
    return _cache[key]


def pair2(name: str):
    if ("pair2", name) not in _cache:
        _cache[("pair2", name)] = synth.make_pair(1) if name == "room8" else synth.make_pair(2, n_tgt=20_000, n_src=20_000)
    return _cache[("pair2", name)]


def maps2(name: str, cell: float = 0.5):
    key = ("maps2", name, cell)
    if key not in _cache:
        d = pair2(name)
        prm = O2.NdtParams(cell_size=cell)
        tgt, _ = R2.build_map(d["tx"], d["ty"], prm)
        _, comps = R2.build_map(d["sx"], d["sy"], prm)
        _cache[key] = (tgt, comps, prm)
    return _cache[key]


# ---- the lists of "against the restatement": name -> (dimension, pair, cell size, seed, components)
NEAR_CASES = {
    "3d_small_1m": (3, "small", 1.0, 30251, 1198),
    "2d_room8": (2, "room8", 0.5, 30252, 116),
    "2d_room50": (2, "room50", 0.5, 30252, 1065),
    "2d_room50_fine": (2, "room50", 0.25, 30252, 2135),
    "2d_room50_coarse": (2, "room50", 1.0, 30252, 530),
}


def near_case(name):
    """(target grid, components, parameters, poses [129, P]) of a NEAR_CASES entry."""
    dim, pair, cell, seed, n_comp = NEAR_CASES[name]
    if dim == 3:
        tgt, comps, prm = maps3(pair, cell)
        poses = near_list(POSE3, SPREAD3, seed)
    else:
        tgt, comps, prm = maps2(pair, cell)
        poses = near_list(pair2(pair)["pose"], SPREAD2, seed)
    assert comps.n == n_comp, (name, comps.n)
    return tgt, comps, prm, poses


# ---- the loop closure: a planar guess, and the list over z, roll and pitch round it
def loop_guess3():
    p = LOOP_POSE3
    return (p[0] + 0.05, p[1] - 0.04, 0.0, 0.0, 0.0, p[5] + 0.005)


def loop_list3() -> np.ndarray:
    """11 x 11 x 11 = 1331 poses: z in guess +- 0.5 (step 0.1), roll and pitch in +-0.10 (step 0.02), x, y, yaw the guess's."""
    g = loop_guess3()
    zs = [g[2] + 0.1 * i for i in range(-5, 6)]
    an = [0.02 * i for i in range(-5, 6)]
    return np.array([(g[0], g[1], z, r, p, g[5]) for z in zs for r in an for p in an], dtype=np.float64)
