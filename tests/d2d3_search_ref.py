"""The score volume of the 3D map-to-map pose search by the float64 restatement (docs/ALGORITHM.md section 2.16).

TEST INFRASTRUCTURE ONLY (imported by tests/test_d2d3_search_ref.py and tests/test_gpu_search_map3d.py).  volume() is
d2d3_ref.evaluate(..., mirror32=False)[2] at every pose of search.lattice(window) with z, roll and pitch pinned to the
window centre's, vectorised per yaw: the covariances rotated once per yaw, the voxel of every component by the
contract's float32 rule (d2d3_ref.lookup: float32 records, evaluate_block3's fmaf order), the terms and the sum in
float64.  volume_by_loop() is that sentence taken literally, pose by pose; the CPU test holds the two together.
"""
from __future__ import annotations

import numpy as np

import d2d3_ref as R
from gtsam_ndt_amd import search
from oracle import ndt2d as O2
from oracle import ndt3d as O


def _pose(window, x, y, yaw):
    c = window[0]
    return (float(x), float(y), float(c[2]), float(c[3]), float(c[4]), float(yaw))


def volume_by_loop(tgt: O.Grid3D, comps: R.Components3, window, prm: O.Ndt3Params, mirror32: bool = False) -> np.ndarray:
    xs, ys, th = search.lattice(window)
    vol = np.zeros((th.size, ys.size, xs.size))
    for j, t in enumerate(th):
        for iy, y in enumerate(ys):
            for ix, x in enumerate(xs):
                vol[j, iy, ix] = R.evaluate(tgt, comps, _pose(window, x, y, t), prm, mirror32)[2]
    return vol


def volume(tgt: O.Grid3D, comps: R.Components3, window, prm: O.Ndt3Params) -> np.ndarray:
    """float64 [n_yaw, n_y, n_x]: the restatement's score at every lattice pose."""
    xs, ys, th = search.lattice(window)
    vol = np.zeros((th.size, ys.size, xs.size))
    if comps.n < 1 or tgt.n_valid < 1:
        return vol
    tcov = R.cov_from_icov(tgt.icov)                        # [ncell, 6], zeros where invalid
    tmean = tgt.mean
    Sg = R.sym6_to_mat(comps.cov)                           # [n, 3, 3]
    m64 = comps.mean
    m32 = R._f32(m64)
    x32, y32 = xs.astype(np.float32), ys.astype(np.float32)
    cz = float(window[0][2])
    for j, t in enumerate(th):
        pose = _pose(window, 0.0, 0.0, t)
        R64 = O.rot_and_derivs(*pose[3:])[0]
        R32 = R64.astype(np.float32)
        # ---- the voxel: d2d3_ref.lookup over [ny, nx, n]
        rz = O2._fma32(m32[:, 0], R32[2, 0], O2._fma32(m32[:, 1], R32[2, 1], O2._fma32(m32[:, 2], R32[2, 2], np.float32(cz))))
        px = O2._fma32(m32[:, 0], R32[0, 0], O2._fma32(m32[:, 1], R32[0, 1], O2._fma32(m32[:, 2], R32[0, 2], x32[None, :, None])))
        py = O2._fma32(m32[:, 0], R32[1, 0], O2._fma32(m32[:, 1], R32[1, 1], O2._fma32(m32[:, 2], R32[1, 2], y32[:, None, None])))
        px, py, pz = np.broadcast_arrays(px, py, rz[None, None, :])
        P = np.stack([px, py, pz], axis=-1).reshape(-1, 3)
        key, inside = O.cell_keys3(P, tgt.o, tgt.inv_c, tgt.dims)
        hit = (inside & tgt.valid[key]).reshape(px.shape)
        key = key.reshape(px.shape)
        if not hit.any():
            continue
        # ---- the terms: d2d3_ref.evaluate, mirror32=False, on the hits only
        S = R.mat_to_sym6(R64 @ Sg @ R64.T)                 # [n, 6], once per yaw
        rm = m64 @ R64.T                                    # R mu
        iy, ix, ic = np.nonzero(hit)
        k = key[iy, ix, ic]
        A = S[ic] + tcov[k]
        axx, axy, axz, ayy, ayz, azz = (A[:, q] for q in range(6))
        c00 = ayy * azz - ayz * ayz
        c01 = axz * ayz - axy * azz
        c02 = axy * ayz - axz * ayy
        c11 = axx * azz - axz * axz
        c12 = axy * axz - axx * ayz
        c22 = axx * ayy - axy * axy
        rdet = 1.0 / (axx * c00 + (axy * c01 + axz * c02))
        q0 = rm[ic, 0] + xs[ix] - tmean[k, 0]
        q1 = rm[ic, 1] + ys[iy] - tmean[k, 1]
        q2 = rm[ic, 2] + cz - tmean[k, 2]
        v0 = (c00 * q0 + (c01 * q1 + c02 * q2)) * rdet
        v1 = (c01 * q0 + (c11 * q1 + c12 * q2)) * rdet
        v2 = (c02 * q0 + (c12 * q1 + c22 * q2)) * rdet
        mm = q0 * v0 + (q1 * v1 + q2 * v2)
        with np.errstate(under="ignore"):
            s = prm.d1 * np.exp(-0.5 * prm.d2 * mm)
        np.add.at(vol[j], (iy, ix), s)
    return vol
