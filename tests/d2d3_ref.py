"""float64 restatement of 3D map-to-map alignment (distribution-to-distribution NDT), docs/ALGORITHM.md §2.14.

TEST INFRASTRUCTURE ONLY (imported by tests/test_d2d3_ref.py and tests/test_gpu_d2d3.py): built on
oracle.ndt3d.build_grid3 for both maps, on rot_and_derivs / rot_second_derivs for the definition of the
derivatives and on oracle.ndt3d.gn_update3 for the step, so everything but the per-component terms is the code the
point-to-map tests already trust.

A *component* is a valid voxel of a grid: its mean and its regularised covariance, the float64 inverse of the
`icov` the oracle stores.  The source map is its component list in voxel-key order, the target map is looked up
at the float32 image of the component's mean (float32 records, evaluate_block3's fmaf order) in both modes below,
so the two modes see the same pairs:
  mirror32=False  the truth: float64 means and covariances, float64 arithmetic
  mirror32=True   the float32 records and every per-component operation rounded to float32 (the order the
                  kernel uses, without its fma contraction), summed in float64; what the GPU tests take their
                  bound from

Two statements of the terms live here.  evaluate() is the one the kernel implements: the map-frame form, where
dR/da_k = [a_k]x R with a_roll = R[:, 0], a_pitch = Rz e_y, a_yaw = e_z, so that
Z_k v = a_k x (S v) - S (a_k x v) and d2R/da_k da_l = [a_l]x [a_k]x R for k <= l.  evaluate_by_definition() forms
j_a, Z_a, j_ab, Z_ab from the oracle's derivative matrices exactly as §2.14 writes them; tests/test_d2d3_ref.py
holds the two against each other and against central differences.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from oracle import ndt2d as O2
from oracle import ndt3d as O

SYM = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # xx xy xz yy yz zz


@dataclass
class Components3:
    key: np.ndarray     # int64 [n]   voxel keys (iz H + iy) W + ix, ascending
    mean: np.ndarray    # float64 [n, 3]
    cov: np.ndarray     # float64 [n, 6]  (xx xy xz yy yz zz) of the regularised covariance

    @property
    def n(self) -> int:
        return int(self.key.shape[0])


def sym6_to_mat(c6: np.ndarray) -> np.ndarray:
    M = np.empty(c6.shape[:-1] + (3, 3), dtype=c6.dtype)
    for q, (i, j) in enumerate(SYM):
        M[..., i, j] = c6[..., q]
        M[..., j, i] = c6[..., q]
    return M


def mat_to_sym6(M: np.ndarray) -> np.ndarray:
    return np.stack([M[..., i, j] for i, j in SYM], axis=-1)


def cov_from_icov(icov6: np.ndarray) -> np.ndarray:
    """(xx .. zz) of Sigma^-1 -> (xx .. zz) of Sigma, float64; rows of zeros stay zeros."""
    out = np.zeros_like(icov6, dtype=np.float64)
    ok = np.any(icov6 != 0.0, axis=1)
    if ok.any():
        inv = np.linalg.inv(sym6_to_mat(icov6[ok].astype(np.float64)))
        out[ok] = mat_to_sym6(0.5 * (inv + np.swapaxes(inv, -1, -2)))
    return out


def components(grid: O.Grid3D) -> Components3:
    k = np.nonzero(grid.valid)[0].astype(np.int64)          # ascending = voxel-key order
    return Components3(k, grid.mean[k].copy(), cov_from_icov(grid.icov[k]))


def build_map(x, y, z, prm: O.Ndt3Params):
    """(grid, components) of a point set: what a handle holds after set_target."""
    g = O.build_grid3(x, y, z, prm)
    return g, components(g)


def _f32(a):
    return np.asarray(a, dtype=np.float32)


def lookup(tgt: O.Grid3D, comps: Components3, pose):
    """Target voxel of every source component at `pose` by the contract's float32 rule.  Returns
    (key int64 [n], hit bool [n], P32 float32 [n, 3])."""
    R = O.rot_and_derivs(*pose[3:])[0].astype(np.float32)
    t = _f32(pose[:3])
    m = _f32(comps.mean)
    P = np.stack([O2._fma32(m[:, 0], R[r, 0], O2._fma32(m[:, 1], R[r, 1], O2._fma32(m[:, 2], R[r, 2], t[r])))
                  for r in range(3)], axis=1)
    key, inside = O.cell_keys3(P, tgt.o, tgt.inv_c, tgt.dims)
    hit = inside & tgt.valid[key]
    return key, hit, P


def _axes(pose):
    """a_roll, a_pitch, a_yaw (float64): dR/da_k = [a_k]x R."""
    R = O.rot_and_derivs(*pose[3:])[0]
    cg, sg = math.cos(pose[5]), math.sin(pose[5])
    return [R[:, 0].copy(), np.array([-sg, cg, 0.0]), np.array([0.0, 0.0, 1.0])]


def _dot3(a, b):
    """a . b per row in the kernel's nesting: a0 b0 + (a1 b1 + a2 b2)."""
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def _cross(a, b):
    """a x b, a = three scalars, b = three arrays."""
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _symv(S, x):
    """S x for S = (xx xy xz yy yz zz) arrays."""
    return [_dot3((S[0], S[1], S[2]), x), _dot3((S[1], S[3], S[4]), x), _dot3((S[2], S[4], S[5]), x)]


def _assemble(terms, w, n_hit, s):
    """29 per-component terms x weights -> H (6x6), g, score, n_hit; summed in float64."""
    f64sum = lambda a: float(np.sum((w * a).astype(np.float64)))
    tot = [f64sum(a) for a in terms]
    H = np.zeros((6, 6))
    for q, (i, j) in enumerate(SYM):
        H[i, j] = H[j, i] = tot[q]
    for r in range(3):
        for k in range(3):
            H[r, 3 + k] = H[3 + k, r] = tot[6 + 3 * r + k]
    for q, (k, l) in enumerate(SYM):
        H[3 + k, 3 + l] = H[3 + l, 3 + k] = tot[15 + q]
    g = np.array(tot[21:27])
    return H, g, float(np.sum(s.astype(np.float64))), n_hit


def evaluate(tgt: O.Grid3D, comps: Components3, pose, prm: O.Ndt3Params, mirror32: bool = False, pairs: list | None = None):
    """H (6x6), g (6), score, n_hit of f = -sum_i d1 exp(-d2/2 q' (R S_i R' + S_j)^-1 q) at `pose`.
    pairs (optional list): receives the array of target keys per component (-1: no hit)."""
    pose = tuple(float(v) for v in pose)
    key, hit, P32 = lookup(tgt, comps, pose)
    if pairs is not None:
        pairs.append(np.where(hit, key, -1))
    k = key[hit]
    n_hit = int(hit.sum())
    R64 = O.rot_and_derivs(*pose[3:])[0]
    ax64 = _axes(pose)
    tcov = cov_from_icov(tgt.icov[k])
    if mirror32:
        F = np.float32
        R = R64.astype(F)
        t = _f32(pose[:3])
        ax = [a.astype(F) for a in ax64]
        p = [P32[hit, c] for c in range(3)]
        Sg = [_f32(comps.cov[hit, q]) for q in range(6)]
        mj = [tgt.records32()[0][k, c] for c in range(3)]
        Tj = [_f32(tcov[:, q]) for q in range(6)]
        d1, d2 = F(prm.d1), F(prm.d2)
    else:
        F = np.float64
        R = R64
        t = np.array(pose[:3])
        ax = ax64
        m = comps.mean[hit]
        p = [R[r, 0] * m[:, 0] + R[r, 1] * m[:, 1] + R[r, 2] * m[:, 2] + t[r] for r in range(3)]
        Sg = [comps.cov[hit, q] for q in range(6)]
        mj = [tgt.mean[k, c] for c in range(3)]
        Tj = [tcov[:, q] for q in range(6)]
        d1, d2 = prm.d1, prm.d2
    half = F(0.5)
    Sm = [[Sg[0], Sg[1], Sg[2]], [Sg[1], Sg[3], Sg[4]], [Sg[2], Sg[4], Sg[5]]]
    # T = R Sigma, S = T R' (six entries)
    T = [[_dot3((R[r, 0], R[r, 1], R[r, 2]), (Sm[0][c], Sm[1][c], Sm[2][c])) for c in range(3)] for r in range(3)]
    S = [_dot3(T[i], (R[j, 0], R[j, 1], R[j, 2])) for i, j in SYM]
    A = [S[q] + Tj[q] for q in range(6)]
    axx, axy, axz, ayy, ayz, azz = A
    c00 = ayy * azz - ayz * ayz
    c01 = axz * ayz - axy * azz
    c02 = axy * ayz - axz * ayy
    c11 = axx * azz - axz * axz
    c12 = axy * axz - axx * ayz
    c22 = axx * ayy - axy * axy
    rdet = F(1.0) / _dot3((axx, axy, axz), (c00, c01, c02))
    B = [c00 * rdet, c01 * rdet, c02 * rdet, c11 * rdet, c12 * rdet, c22 * rdet]
    q = [p[c] - mj[c] for c in range(3)]
    v = _symv(B, q)
    mm = _dot3(q, v)
    s = d1 * np.exp(-half * d2 * mm)
    w = s * d2
    Sv = _symv(S, v)
    pr = [p[c] - t[c] for c in range(3)]
    jk, pk, ek, fk, rk, ck, Uk = [], [], [], [], [], [], []
    for a in ax:
        j = _cross(a, pr)
        pp = _cross(a, v)
        e = _cross(a, Sv)
        f = _symv(S, pp)
        z = [e[c] - f[c] for c in range(3)]
        r = [j[c] - z[c] for c in range(3)]
        jk.append(j); pk.append(pp); ek.append(e); fk.append(f); rk.append(r)
        ck.append(_dot3(v, j) - half * _dot3(v, z))
        Uk.append(_symv(B, r))
    newton = prm.hessian_mode == 1
    terms = []
    for qi, (i, j) in enumerate(SYM):                                   # Htt
        terms.append(B[qi] - d2 * v[i] * v[j] if newton else B[qi])
    for r in range(3):                                                  # Htr
        for kk in range(3):
            terms.append(Uk[kk][r] - d2 * v[r] * ck[kk] if newton else Uk[kk][r])
    for kk, ll in SYM:                                                  # Hrr, k <= l
        h = _dot3(rk[kk], Uk[ll])
        if newton:
            ej = [ek[kk][c] - jk[kk][c] for c in range(3)]
            h = (h - d2 * ck[kk] * ck[ll]) + (_dot3(pk[ll], ej) - _dot3(pk[kk], fk[ll]))
        terms.append(h)
    terms += [v[0], v[1], v[2], ck[0], ck[1], ck[2]]
    return _assemble(terms, w, n_hit, s)


def evaluate_by_definition(tgt: O.Grid3D, comps: Components3, pose, prm: O.Ndt3Params):
    """The same quantities from §2.14 as written: j_a, Z_a, j_ab, Z_ab formed from oracle.ndt3d's derivative
    matrices, float64, one matrix product at a time (slow; for tests)."""
    pose = tuple(float(v) for v in pose)
    key, hit, _ = lookup(tgt, comps, pose)
    k = key[hit]
    R, Ra, Rb, Rg = O.rot_and_derivs(*pose[3:])
    dd = O.rot_second_derivs(*pose[3:])
    Rd = [Ra, Rb, Rg]
    t = np.array(pose[:3])
    mu = comps.mean[hit]
    Sg = sym6_to_mat(comps.cov[hit])
    Sj = sym6_to_mat(cov_from_icov(tgt.icov[k]))
    S = R @ Sg @ R.T
    B = np.linalg.inv(S + Sj)
    q = mu @ R.T + t - tgt.mean[k]
    v = np.einsum("nij,nj->ni", B, q)
    s = prm.d1 * np.exp(-0.5 * prm.d2 * np.einsum("ni,ni->n", q, v))
    w = s * prm.d2
    n = mu.shape[0]
    j = np.zeros((6, n, 3))
    Z = np.zeros((6, n, 3, 3))
    for a in range(3):
        j[a, :, a] = 1.0
        j[3 + a] = mu @ Rd[a].T
        Z[3 + a] = Rd[a] @ Sg @ R.T + R @ Sg @ Rd[a].T
    Zv = np.einsum("anij,nj->ani", Z, v)
    r = j - Zv
    c = np.einsum("ni,ani->an", v, j - 0.5 * Zv)
    g = np.einsum("n,an->a", w, c)
    H = np.einsum("n,ani,nij,bnj->ab", w, r, B, r)
    if prm.hessian_mode == 1:
        H = H - prm.d2 * np.einsum("n,an,bn->ab", w, c, c)
        for (a, b), Rab in dd.items():
            jab = mu @ Rab.T
            Zab = Rab @ Sg @ R.T + Rd[a] @ Sg @ Rd[b].T + Rd[b] @ Sg @ Rd[a].T + R @ Sg @ Rab.T
            t2 = float(np.sum(w * (np.einsum("ni,ni->n", v, jab) - 0.5 * np.einsum("ni,nij,nj->n", v, Zab, v))))
            H[3 + a, 3 + b] += t2
            if a != b:
                H[3 + b, 3 + a] += t2
    return H, g, float(s.sum()), int(hit.sum())


def score(tgt, comps, pose, prm) -> float:
    return evaluate(tgt, comps, pose, prm)[2]


def align(tgt: O.Grid3D, comps: Components3, init_pose, prm: O.Ndt3Params, mirror32: bool = False, trace: list | None = None):
    """The loop of oracle.ndt3d.align3 over the map-to-map terms; the result's H, g, score, n_hit are the last evaluation's."""
    pose = tuple(float(v) for v in init_pose)
    it = 0
    if comps.n < 1 or tgt.n_valid < 1:
        return {"pose": pose, "H": np.zeros((6, 6)), "g": np.zeros(6), "score": 0.0, "n_hit": 0, "iterations": 0,
                "status": O.NDT_TOO_FEW_CELLS}
    ls = {} if prm.line_search > 0 else None
    while True:
        H, g, sc, n_hit = evaluate(tgt, comps, pose, prm, mirror32)
        if trace is not None:
            trace.append({"pose": pose, "H": H.copy(), "g": g.copy(), "score": sc, "n_hit": n_hit})
        pose, it, status, done = O.gn_update3(pose, H, g, n_hit, it, prm, sc, ls)
        if done:
            return {"pose": pose, "H": H, "g": g, "score": sc, "n_hit": n_hit, "iterations": it, "status": status}


# ---- how two evaluations are compared (the normalisation of tests/d2d_ref.py) ---------------------------------
def eval_diffs(a, b, Hgn=None):
    """(H, g, score) differences of evaluation a against the reference b, each relative to its natural scale:
    H entry (i, j) to sqrt(H_ii H_jj), g_i to sqrt(H_ii * score) (its entries cancel), the score to itself.  The
    diagonal is the Gauss-Newton one (Hgn, positive) when given, else b's own."""
    Ha, ga, sa, _ = a
    Hb, gb, sb, _ = b
    d = np.sqrt(np.abs(np.diag(Hb if Hgn is None else Hgn))) + 1e-300
    return (float(np.max(np.abs(Ha - Hb) / np.outer(d, d))), float(np.max(np.abs(ga - gb) / (d * math.sqrt(max(sb, 1.0))))),
            abs(sa - sb) / sb)


EVAL_FLOOR = 2e-5       # the project's bound on H / g against the mirror oracle


def eval_bounds(cases, prm):
    """The GPU tests' bound on (H, g, score), measured from this restatement alone: 4 x the largest
    float32-vs-float64 difference over `cases` = [(tgt, comps, pose)], floored at EVAL_FLOOR.
    Returns (bounds [3], measured [3])."""
    gn = O.Ndt3Params(**{**prm.__dict__, "hessian_mode": 0})
    worst = np.zeros(3)
    for tgt, comps, pose in cases:
        Hgn = evaluate(tgt, comps, pose, gn)[0]
        d = eval_diffs(evaluate(tgt, comps, pose, prm, mirror32=True), evaluate(tgt, comps, pose, prm), Hgn)
        worst = np.maximum(worst, d)
    return np.maximum(4.0 * worst, EVAL_FLOOR), worst
