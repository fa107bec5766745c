"""The float64 restatement of 3D map-to-map alignment (tests/d2d3_ref.py; docs/ALGORITHM.md section 2.14) is right by
its own finite differences and by the section's formulas taken literally, a map against itself stays where it is, two
scans of one scene a known transform apart are brought together, and the three entry points exist in the header, the
library and the bindings.

Measured here (float64, Newton mode, five poses per scene with the voxel lookup in play): central differences of the
score reproduce g to 5.0e-10 of sqrt(H_aa score) and central differences of g reproduce the Newton H to 3.9e-9 of
sqrt(H_aa H_bb) (H_aa of the Gauss-Newton form); the map-frame form agrees with the by-definition form to 2e-14.
Asserted a small factor above: 2e-8 for the differences, 1e-10 for the two forms."""
import os
import re

import numpy as np
import pytest

import d2d3_ref as R
from gtsam_ndt_amd import synth3d
from oracle import ndt3d as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE_A = (0.10, -0.08, 0.02, 0.004, -0.003, 0.01)
# name -> (generating pose or None for the stock pair, cell size); both at n_elev = 32, n_azim = 1024 to keep the CPU suite short
SCENES = {"near1m": (POSE_A, 1.0), "stock2m": (None, 2.0)}
NAMES = ("ndt3d_evaluate_map", "ndt3d_align_map", "ndt3d_get_components")
FD_BOUND = 2e-8


def _maps(scene, **opts):
    pose, cell = SCENES[scene]
    kw = dict(n_elev=32, n_azim=1024)
    d = synth3d.make_pair3d(pose=pose, **kw) if pose is not None else synth3d.make_pair3d(**kw)
    prm = O.Ndt3Params(cell_size=cell, **opts)
    tgt, _ = R.build_map(d["tx"], d["ty"], d["tz"], prm)
    _, comps = R.build_map(d["sx"], d["sy"], d["sz"], prm)
    return d, tgt, comps, prm


def _poses(d, tgt, comps, cell):
    """Five poses: the start, the generating pose, the converged pose and two more off it."""
    conv = R.align(tgt, comps, d["init"], O.Ndt3Params(cell_size=cell))["pose"]
    t = d["pose"]
    return [d["init"], t, conv, tuple(np.array(t) + np.array([0.07, -0.05, 0.03, 0.01, -0.008, 0.012])),
            tuple(np.array(t) + np.array([-0.04, 0.09, -0.02, -0.006, 0.011, -0.02]))]


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_gradient_and_newton_hessian_match_central_differences(scene):
    """Steps: 1e-6 m in translation, 1e-6 m of arc at the farthest component in the angles, so every image moves at
    most about 1e-6 m, under 1e-4 of the narrowest Gaussian a default voxel holds: the truncation term of a central
    difference is below 1e-8 of the differentiated quantity's scale, the float64 rounding term eps x sum / step of the
    same order.  No component may change its target voxel inside the stencil."""
    d, tgt, comps, prm = _maps(scene, hessian_mode=1)
    gn = O.Ndt3Params(cell_size=prm.cell_size)
    arm = float(np.linalg.norm(comps.mean, axis=1).max())
    step = (1e-6, 1e-6, 1e-6, 1e-6 / arm, 1e-6 / arm, 1e-6 / arm)
    worst = np.zeros(3)
    for pose in _poses(d, tgt, comps, prm.cell_size):
        pairs = []
        H, g, sc, n_hit = R.evaluate(tgt, comps, pose, prm, pairs=pairs)
        Hgn = R.evaluate(tgt, comps, pose, gn)[0]
        assert n_hit >= 0.5 * comps.n
        gf, Hf = np.zeros(6), np.zeros((6, 6))
        for a in range(6):
            pp, pm = list(pose), list(pose)
            pp[a] += step[a]
            pm[a] -= step[a]
            ep, em = R.evaluate(tgt, comps, pp, prm, pairs=pairs), R.evaluate(tgt, comps, pm, prm, pairs=pairs)
            gf[a] = -(ep[2] - em[2]) / (2 * step[a])            # f = -score
            Hf[:, a] = (ep[1] - em[1]) / (2 * step[a])
        for other in pairs[1:]:
            assert np.array_equal(pairs[0], other), "a component changed its target voxel inside the difference stencil"
        dg = np.sqrt(np.diag(Hgn))
        eg = np.abs(gf - g) / (dg * np.sqrt(sc))
        eh = np.abs(Hf - H) / np.outer(dg, dg)
        by_def = R.evaluate_by_definition(tgt, comps, pose, prm)
        ed = max(R.eval_diffs((H, g, sc, n_hit), by_def, Hgn))
        worst = np.maximum(worst, [eg.max(), eh.max(), ed])
        print(f"{scene} pose {np.round(pose, 4)}: n_hit {n_hit}, |g_fd - g| {eg.max():.2e}, |H_fd - H| {eh.max():.2e}, "
              f"map-frame form vs definition {ed:.2e} (scaled)")
        assert eg.max() < FD_BOUND and eh.max() < FD_BOUND
        assert ed < 1e-10 and by_def[3] == n_hit
        assert np.abs(H - H.T).max() == 0.0
    print(f"{scene}: worst (g, H, forms) {worst}")


@pytest.mark.parametrize("scene", sorted(SCENES))
def test_gauss_newton_hessian_is_symmetric_positive_semidefinite(scene):
    d, tgt, comps, prm = _maps(scene)
    for pose in _poses(d, tgt, comps, prm.cell_size):
        H = R.evaluate(tgt, comps, pose, prm)[0]
        assert np.array_equal(H, H.T)
        dg = np.sqrt(np.diag(H))
        ev = np.linalg.eigvalsh(H / np.outer(dg, dg))
        assert ev.min() >= -1e-12 * ev.max(), ev


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_a_map_against_itself_stays_at_the_identity(scene, mode):
    d, _, _, prm = _maps(scene, hessian_mode=mode)
    tgt, comps = R.build_map(d["tx"], d["ty"], d["tz"], prm)
    zero = (0.0,) * 6
    for mirror in (False, True):
        H, g, sc, n_hit = R.evaluate(tgt, comps, zero, prm, mirror32=mirror)
        assert n_hit == comps.n                                  # every mean sits on its own voxel's mean: q = 0
        assert not g.any()                                       # ... so v = 0 and every gradient term is an exact zero
        assert sc == pytest.approx(prm.d1 * comps.n, rel=1e-6)
    r = R.align(tgt, comps, zero, prm)
    assert r["status"] == O.NDT_OK and r["iterations"] == 1 and r["pose"] == zero


def test_components_are_in_key_order_and_invert_the_oracle_records():
    for scene in sorted(SCENES):
        _, tgt, _, _ = _maps(scene)
        comps = R.components(tgt)
        assert comps.n == tgt.n_valid and np.all(np.diff(comps.key) > 0)
        prod = R.sym6_to_mat(comps.cov) @ R.sym6_to_mat(tgt.icov[comps.key])
        err = np.abs(prod - np.eye(3)).max()
        print(f"{scene}: {comps.n} components, |Sigma Sigma^-1 - I| {err:.2e}")
        assert err < 1e-10


@pytest.mark.parametrize("opts", [dict(), dict(line_search=4)], ids=["plain", "linesearch4"])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_two_scans_a_known_transform_apart_converge(scene, opts):
    """From the zero guess, Gauss-Newton.  The maps are two independent samplings summarised per voxel: the optimum is
    asked to lie within a twentieth of a voxel and 5 mrad of the generating pose, not closer (measured: 1 cm, 1 mrad)."""
    d, tgt, comps, prm = _maps(scene, **opts)
    r = R.align(tgt, comps, d["init"], prm)
    err = np.abs(np.array(r["pose"]) - np.array(d["pose"]))
    print(f"{scene} {opts}: {r['iterations']} iterations, status {r['status']}, |pose - truth| {err}")
    assert r["status"] == O.NDT_OK
    assert err[:3].max() < 0.05 * prm.cell_size and err[3:].max() < 5e-3
    assert r["n_hit"] >= 0.5 * comps.n


def test_float32_restatement_tracks_the_float64_one():
    """What the GPU tests take their bound from: the per-component arithmetic in float32 against float64 (measured on
    these scenes: 8.7e-6 for H, 8.3e-6 for g, 4.5e-7 for the score)."""
    for scene in sorted(SCENES):
        d, tgt, comps, prm = _maps(scene, hessian_mode=1)
        gn = O.Ndt3Params(cell_size=prm.cell_size)
        for pose in _poses(d, tgt, comps, prm.cell_size)[:3]:
            a, b = R.evaluate(tgt, comps, pose, prm, mirror32=True), R.evaluate(tgt, comps, pose, prm)
            diffs = R.eval_diffs(a, b, R.evaluate(tgt, comps, pose, gn)[0])
            print(f"{scene} pose {np.round(pose, 4)}: float32 vs float64 (H, g, score) {diffs}")
            assert a[3] == b[3] and max(diffs) < 1e-4


def test_the_three_entry_points_are_declared_exported_and_bound(ndt_lib):
    from gtsam_ndt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ndt_hip.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint32_t\s+%s\s*\(" % n, src), f"{n} is not declared in ndt_hip.h"
        assert hasattr(ndt_lib, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is not bound"
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    for m in ("align_map", "evaluate_map", "components"):
        assert callable(getattr(NdtMatcher3D, m))
    import adapter_calls as AC                                  # the C++ adapter's call record
    assert "ndt3d_align_map" in AC.calls()["NdtMatcherHip3.alignMap"]
