"""The restatement of the map-to-map score at a list of poses (tests/d2d_pose_list_ref.py) on the CPU: held to the
restated search volumes on a lattice given as a list, its float32 form held to its float64 form on the lists the GPU
tests score, and the loop closure over z, roll and pitch that the (x, y, yaw) lattice cannot do.

The bound of the GPU tests is the project's for a private-sum float32 score, 1e-4 |ref| + 1e-3
(tests/test_gpu_search_map*.py).  It stays supported by the restatement alone while the float32 form uses at most a
quarter of it; the worst shares measured here are in WORST_SHARE."""
import math

import numpy as np
import pytest

import d2d3_ref as R3
import d2d3_search_ref as S3
import d2d_pose_list_ref as P
import d2d_search_ref as S2
from gtsam_ndt_amd import search
from oracle import ndt3d as O3

DEG = math.pi / 180.0
# name: (worst |float32 - float64| / (1e-4 |float64| + 1e-3) over the list, largest float64 score), as measured
WORST_SHARE = {
    "3d_small_1m": (0.054, 254.5),
    "2d_room8": (0.008, 69.5),
    "2d_room50": (0.062, 699.0),
    "2d_room50_fine": (0.047, 1216.0),
    "2d_room50_coarse": (0.028, 394.0),
}


def test_a_lattice_list_is_the_restated_volume_2d():
    tgt, comps, prm = P.maps2("room8")
    window = search.Window(P.pair2("room8")["init"], (0.3, 0.2, 0.3), (0.1, 0.1, 0.15))
    ref = S2.volume(tgt, comps, window, prm)
    sc, nh = P.scores2d(tgt, comps, P.lattice_list(window), prm)
    assert sc.shape == (ref.size,) and ref.max() > 10.0
    assert np.all(np.abs(sc - ref.reshape(-1)) <= 1e-9 * np.abs(ref.reshape(-1)))
    assert np.all((nh > 0) == (sc > 0))


def test_a_lattice_list_is_the_restated_volume_3d():
    tgt, comps, prm = P.maps3("small", 2.0)
    c = (P.POSE3[0] + 0.1, P.POSE3[1] - 0.1, 0.1, 0.05, -0.04, P.POSE3[5] + 0.02)
    window = search.Window(c, (0.5, 0.25, 0.1), (0.25, 0.25, 0.1))
    ref = S3.volume(tgt, comps, window, prm)
    poses = P.lattice_list(window)
    assert poses.shape == (ref.size, 6) and np.all(poses[:, 2:5] == np.array(c[2:5]))
    sc, nh = P.scores3d(tgt, comps, poses, prm)
    assert ref.max() > 10.0
    assert np.all(np.abs(sc - ref.reshape(-1)) <= 1e-9 * np.abs(ref.reshape(-1)))
    assert np.all((nh > 0) == (sc > 0))


def test_non_finite_poses_score_zero():
    tgt, comps, prm = P.maps3("small", 2.0)
    poses = np.array([P.POSE3, P.POSE3, P.POSE3], dtype=np.float64)
    poses[0, 2] = math.nan
    poses[2, 5] = math.inf
    sc, nh = P.scores3d(tgt, comps, poses, prm)
    assert sc[0] == 0.0 and sc[2] == 0.0 and nh[0] == 0 and nh[2] == 0 and sc[1] > 10.0 and nh[1] > 0


@pytest.mark.parametrize("name", sorted(P.NEAR_CASES))
def test_the_float32_form_stays_within_a_quarter_of_the_bound(name):
    tgt, comps, prm, poses = P.near_case(name)
    score = P.scores3d if P.NEAR_CASES[name][0] == 3 else P.scores2d
    ref, nh = score(tgt, comps, poses, prm)
    f32, nh32 = score(tgt, comps, poses, prm, mirror32=True)
    share = np.abs(f32 - ref) / (1e-4 * np.abs(ref) + 1e-3)
    print(f"{name}: {comps.n} components, worst share of the bound {share.max():.3f}, max ref {ref.max():.1f}, "
          f"recorded {WORST_SHARE[name]}")
    assert poses.shape[0] == 129 and ref.max() > 10.0
    assert share.max() <= 0.25
    assert np.array_equal(nh, nh32)


def _dist(p, q):
    dt = math.sqrt(sum((p[a] - q[a]) ** 2 for a in range(3)))
    return dt, max(abs(float(search.wrap(p[a] - q[a]))) for a in range(3, 6))


def test_a_list_over_z_roll_and_pitch_closes_a_loop_the_planar_guess_cannot():
    """Two 3D submaps whose relative height (0.35 m) and tilt (0.07, -0.05 rad) are unknown: align from the planar guess
    ends 0.342 m / 0.072 rad off (score 125.1); the best of the 1331 poses over z, roll and pitch scores 151.3 against
    83.4 at the guess, and align from it ends 0.011 m / 4.5e-4 rad off (score 279.0)."""
    tgt, comps, prm = P.maps3("small", 1.0, P.LOOP_POSE3)
    assert comps.n == 1326
    guess = P.loop_guess3()
    local = R3.align(tgt, comps, guess, prm)
    dt, dr = _dist(local["pose"], P.LOOP_POSE3)
    print(f"from the planar guess: status {local['status']}, {dt:.3f} m / {dr:.3f} rad off, score {local['score']:.1f}")
    assert local["status"] == O3.NDT_OK and dt > 0.3
    poses = P.loop_list3()
    assert poses.shape == (1331, 6)
    sc, _ = P.scores3d(tgt, comps, poses, prm)
    best = int(np.argmax(sc))
    at_guess = R3.evaluate(tgt, comps, guess, prm)[2]
    print(f"best of the list: {tuple(poses[best])} scores {sc[best]:.1f}, the guess {at_guess:.1f}")
    assert np.allclose(poses[best], P.LOOP_BEST3, rtol=0.0, atol=1e-12)
    assert sc[best] > 1.5 * at_guess
    fine = R3.align(tgt, comps, tuple(poses[best]), prm)
    dt, dr = _dist(fine["pose"], P.LOOP_POSE3)
    print(f"from the best pose: status {fine['status']}, {dt:.4f} m / {dr:.2e} rad off, score {fine['score']:.1f}")
    assert fine["status"] == O3.NDT_OK and dt < 0.05 and dr < 0.005
