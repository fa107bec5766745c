"""The float64 restatement of the map neighbourhood (tests/d2d3_nb_ref.py; docs/ALGORITHM.md section 2.26) without a
device: at 1 it is tests/d2d3_ref.py, at 7 it is right by its own central differences, candidates are taken by index, and
it does what the option is for - the stock pair at 1 m voxels from the zero guess ends 0.3 m from the generating pose
with the own voxel alone and within millimetres of it with the six face neighbours.

Measured here (float64 unless said): near1m at 7, five poses, central differences reproduce g to 3.8e-10 of
sqrt(H_aa score) and the Newton H to 3.7e-9 of sqrt(H_aa H_bb) (bound: tests/test_d2d3_ref.py's 2e-8).  Stock pair (64 x 2048, 2 180 components against 2 706
voxels): with 1, 34 iterations, NDT_OK, 0.326 m / 28 mrad from the generating pose; with 7, 68 iterations, NDT_OK,
1.6 mm / 0.24 mrad, n_hit 10 497; the float32-mirrored run at 7 takes the same 68 iterations and ends 9e-8 m / 1e-8 rad
from the float64 one."""
import numpy as np
import pytest

import d2d3_nb_ref as NB
import d2d3_ref as R
import test_d2d3_ref as T
from gtsam_ndt_amd import synth3d
from oracle import ndt3d as O

ZERO = (0.0,) * 6


@pytest.mark.parametrize("mode", [0, 1])
def test_at_one_it_is_the_single_voxel_restatement(mode):
    d, tgt, comps, prm = T._maps("near1m", hessian_mode=mode)
    for pose in (d["init"], d["pose"]):
        for mirror in (False, True):
            a, b = NB.evaluate_nb(tgt, comps, pose, prm, 1, mirror), R.evaluate(tgt, comps, pose, prm, mirror)
            assert a[3] == b[3] > 0
            assert np.abs(a[0] - b[0]).max() <= 1e-12 * np.abs(b[0]).max()
            assert np.abs(a[1] - b[1]).max() <= 1e-12 * np.abs(b[0]).max() and abs(a[2] - b[2]) <= 1e-12 * b[2]
    assert R.lookup.__module__ == "d2d3_ref"                       # the candidate's lookup does not outlive its call


def test_gradient_and_newton_hessian_match_central_differences_at_7():
    """test_d2d3_ref.py's stencil and bound, on the sums over the seven candidates.  No candidate of any component may
    change inside the stencil."""
    d, tgt, comps, prm = T._maps("near1m", hessian_mode=1)
    gn = O.Ndt3Params(cell_size=prm.cell_size)
    arm = float(np.linalg.norm(comps.mean, axis=1).max())
    step = (1e-6, 1e-6, 1e-6, 1e-6 / arm, 1e-6 / arm, 1e-6 / arm)
    for pose in T._poses(d, tgt, comps, prm.cell_size):
        own = NB.candidates(tgt, comps, pose, 7)[0]
        H, g, sc, n_hit = NB.evaluate_nb(tgt, comps, pose, prm, 7)
        Hgn = NB.evaluate_nb(tgt, comps, pose, gn, 7)[0]
        assert n_hit > 2 * R.evaluate(tgt, comps, pose, prm)[3]
        gf, Hf = np.zeros(6), np.zeros((6, 6))
        for a in range(6):
            pp, pm = list(pose), list(pose)
            pp[a] += step[a]
            pm[a] -= step[a]
            for q in (pp, pm):
                for (k0, h0), (k1, h1) in zip(own, NB.candidates(tgt, comps, q, 7)[0]):
                    assert np.array_equal(h0, h1) and np.array_equal(k0[h0], k1[h1]), "a candidate changed inside the stencil"
            ep, em = NB.evaluate_nb(tgt, comps, pp, prm, 7), NB.evaluate_nb(tgt, comps, pm, prm, 7)
            gf[a] = -(ep[2] - em[2]) / (2 * step[a])                # f = -score
            Hf[:, a] = (ep[1] - em[1]) / (2 * step[a])
        dg = np.sqrt(np.diag(Hgn))
        eg = np.abs(gf - g) / (dg * np.sqrt(sc))
        eh = np.abs(Hf - H) / np.outer(dg, dg)
        print(f"near1m at 7, pose {np.round(pose, 4)}: n_hit {n_hit}, |g_fd - g| {eg.max():.2e}, |H_fd - H| {eh.max():.2e} (scaled)")
        assert eg.max() < T.FD_BOUND and eh.max() < T.FD_BOUND
        assert np.abs(H - H.T).max() == 0.0
        # the Gauss-Newton form: symmetric positive semi-definite
        assert np.array_equal(Hgn, Hgn.T)
        ev = np.linalg.eigvalsh(Hgn / np.outer(dg, dg))
        assert ev.min() >= -1e-12 * ev.max(), ev


def _edge_maps():
    prm = O.Ndt3Params(cell_size=1.0)
    pts = np.concatenate([NB.voxel_points(v) for v in NB.EDGE_VOXELS])
    tgt, _ = NB.build_map_at(np.zeros(3), NB.EDGE_DIMS, pts[:, 0], pts[:, 1], pts[:, 2], prm)
    assert tgt.n_valid == len(NB.EDGE_VOXELS)
    return prm, tgt


def test_candidates_are_skipped_by_index_on_a_hand_built_grid():
    """Six occupied voxels on the faces of a 6 x 5 x 4 grid, in pairs whose keys are 1, W and 15 W apart: none is a face
    neighbour of another, so a one-component source on any of them scores one pair, not two; one voxel outside the grid
    scores nothing, whatever lies next to it; and a real face neighbour does add its pair."""
    prm, tgt = _edge_maps()
    W, H, D = NB.EDGE_DIMS
    keys = sorted((v[2] * H + v[1]) * W + v[0] for v in NB.EDGE_VOXELS)
    assert keys[2] - keys[1] == 1 and keys[4] - keys[3] == W
    for v in NB.EDGE_VOXELS:
        p = NB.voxel_points(v, seed=9)
        _, comps = NB.build_map_at(np.zeros(3), NB.EDGE_DIMS, p[:, 0], p[:, 1], p[:, 2], prm)
        assert comps.n == 1
        for mirror in (False, True):
            r1, r7 = NB.evaluate_nb(tgt, comps, ZERO, prm, 1, mirror), NB.evaluate_nb(tgt, comps, ZERO, prm, 7, mirror)
            assert r1[3] == r7[3] == 1 and r7[2] == r1[2] > 0, v
        # one voxel outside along every axis the voxel touches a face of
        for a in range(3):
            for sgn, at_face in ((-1.0, v[a] == 0), (1.0, v[a] == NB.EDGE_DIMS[a] - 1)):
                if at_face:
                    pose = [0.0] * 6
                    pose[a] = sgn
                    assert NB.evaluate_nb(tgt, comps, pose, prm, 7)[2:] == (0.0, 0), (v, a, sgn)
    # a component one voxel inside of (5, 1, 1): its own voxel is empty, its +x neighbour is not
    p = NB.voxel_points((4, 1, 1), seed=9)
    _, comps = NB.build_map_at(np.zeros(3), NB.EDGE_DIMS, p[:, 0], p[:, 1], p[:, 2], prm)
    r1, r7 = NB.evaluate_nb(tgt, comps, ZERO, prm, 1), NB.evaluate_nb(tgt, comps, ZERO, prm, 7)
    assert r1[3] == 0 and r7[3] == 1 and r7[2] > 0


@pytest.fixture(scope="module")
def stock():
    d = synth3d.make_pair3d()
    prm = O.Ndt3Params(cell_size=1.0)
    tgt, _ = R.build_map(d["tx"], d["ty"], d["tz"], prm)
    _, comps = R.build_map(d["sx"], d["sy"], d["sz"], prm)
    return d, prm, tgt, comps


def test_the_stock_pair_from_the_zero_guess_is_recovered_with_7_and_not_with_1(stock):
    """What the option is for.  "Recovered" is the project's own scale: 1 cm / 1 mrad."""
    d, prm, tgt, comps = stock
    r1 = NB.align_nb(tgt, comps, ZERO, prm, 1)
    r7 = NB.align_nb(tgt, comps, ZERO, prm, 7)
    m7 = NB.align_nb(tgt, comps, ZERO, prm, 7, mirror32=True)
    e1, e7, em = NB.pose_error(r1["pose"], d["pose"]), NB.pose_error(r7["pose"], d["pose"]), NB.pose_error(m7["pose"], r7["pose"])
    print(f"stock pair, {comps.n} components against {tgt.n_valid} voxels: with 1 {r1['iterations']} iterations, status {r1['status']}, "
          f"{e1[0]:.4f} m / {e1[1]:.4f} rad from the generating pose, n_hit {r1['n_hit']}; with 7 {r7['iterations']} iterations, "
          f"status {r7['status']}, {e7[0]:.5f} m / {e7[1]:.5f} rad, n_hit {r7['n_hit']}; float32 mirror at 7 {m7['iterations']} "
          f"iterations, {em[0]:.2e} m / {em[1]:.2e} rad from the float64 run")
    assert r1["status"] == r7["status"] == O.NDT_OK
    assert e1[0] > 0.2
    assert e7[0] < 1e-2 and e7[1] < 1e-3
    assert m7["iterations"] == r7["iterations"] and em[0] < 2.5e-5 and em[1] < 2.5e-5


def test_float32_restatement_tracks_the_float64_one_at_7(stock):
    """What the GPU tests take their bound from (measured on the stock pair at 7: 3.0e-6 / 3.3e-6 / 2.2e-7, below the
    project's 2e-5 floor)."""
    d, prm, tgt, comps = stock
    for mode in (0, 1):
        p = O.Ndt3Params(cell_size=1.0, hessian_mode=mode)
        bound, worst = NB.eval_bounds_nb([(tgt, comps, ZERO), (tgt, comps, d["pose"])], p)
        print(f"stock pair at 7, mode {mode}: float32 vs float64 (H, g, score) {worst}, bound {bound}")
        assert np.all(worst < 1e-4) and np.all(bound >= NB.EVAL_FLOOR)
