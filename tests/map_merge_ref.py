"""Reference for ndt2d/ndt3d_merge_map and ndt*_unmerge_map (docs/ALGORITHM.md section 2.18): two save_map blobs and a
pose -> the blob the destination handle saves afterwards, and the number of points dropped outside it.

The contribution of a source cell is float64 arithmetic in ONE fixed operation order, every operation rounded separately
(numpy elementwise float64 / Python floats: no fused multiply-add), followed by one rounding to integers and an exact
integer clamp, so there is exactly one right answer and the GPU tests compare byte for byte, header included.  Built on
map_coarsen_ref.parse / pack / blob_from_points.

Also here: the exact (rational) value of the same contribution with the float64 evaluation error bounded (exact_contribution:
what the conservation test asserts), and an oracle grid from a blob (grid_from_blob: what the quality test aligns against)."""
import math
from fractions import Fraction as Fr

import numpy as np

import map_coarsen_ref as R
from seam_ref import rot3d_products

FIX = 2.0 ** 22


class MergeError(ValueError):
    pass


def pairs_of(dim):
    return [(a, b) for a in range(dim) for b in range(a, dim)]


def rotation(dim, pose):
    """(R [3][3] Python floats, t [3]) as the host forms them: cos / sin from libm (math, not numpy's vector versions) at
    the pose's angles as they are (the host does not wrap them); in 3D the nine products of csrc/ndt_pose.hpp, stated in
    seam_ref.rot3d_products."""
    pose = [float(v) for v in pose]
    Rm = [[0.0] * 3 for _ in range(3)]
    if dim == 2:
        c, s = math.cos(pose[2]), math.sin(pose[2])
        Rm[0][0], Rm[0][1], Rm[1][0], Rm[1][1] = c, -s, s, c
        return Rm, [pose[0], pose[1], 0.0]
    e = rot3d_products(math.sin(pose[3]), math.cos(pose[3]), math.sin(pose[4]), math.cos(pose[4]),
                       math.sin(pose[5]), math.cos(pose[5]))
    return [e[0:3], e[3:6], e[6:9]], pose[:3]


def centres(origin32, ext, c):
    """cell_centre of every index of one axis: fma(i + 0.5, c, (double)origin) - one rounding, done here in rationals."""
    return np.array([float(Fr(2 * i + 1, 2) * Fr(float(c)) + Fr(float(origin32))) for i in range(ext)], dtype=np.float64)


def _row(Rm, r, v, dim):
    acc = Rm[r][0] * v[0] + Rm[r][1] * v[1]
    if dim == 3:
        acc = acc + Rm[r][2] * v[2]
    return acc


def _geometry(h):
    dim = h["dims"]
    ext = [h["width"], h["height"], h["depth"]][:dim]
    org = [np.float32(h["origin"][0][a]) for a in range(dim)]
    return dim, ext, org, float(h["cell_size"])


def contributions(hs, src_cells, hd, pose, clamp=True):
    """Steps 1-3 of section 2.18 for every source cell with 0 < n <= 2^20.  Returns a dict of arrays over those cells:
    k (source cell index), n, cell (destination cell index, -1: outside), on_ring (outside because it landed on the ring), dS [m, dim], dSS [m, npair] (int64), raised
    [m, dim] (what the clamp added to each diagonal second sum) and what exact_contribution needs (the source centres e, the
    integer sums, R, t)."""
    dim, sext, sorg, cs = _geometry(hs)
    dim_d, dext, dorg, cd = _geometry(hd)
    if dim != dim_d or hs["ngrid"] != 1 or hd["ngrid"] != 1:
        raise MergeError("one grid per map, both of one dimension")
    if cs > cd:
        raise MergeError("the source's cell_size exceeds the destination's")
    pairs = pairs_of(dim)
    Rm, t = rotation(dim, pose)
    ring = 1 if dim == 2 else 0
    n_all = src_cells["n"][: int(np.prod(sext))]
    k = np.flatnonzero((n_all > 0) & (n_all <= R.MAX_CELL_COUNT)).astype(np.int64)
    n = n_all[k].astype(np.int64)
    dn = n.astype(np.float64)
    idx = [k % sext[0], (k // sext[0]) % sext[1]] + ([k // (sext[0] * sext[1])] if dim == 3 else [])
    s_fix, d_fix = FIX / cs, FIX / cd
    kk = cs / cd
    kk2 = kk * kk
    S = [src_cells["s"][k, a].astype(np.float64) for a in range(dim)]
    e = [centres(sorg[a], sext[a], cs)[idx[a]] for a in range(dim)]
    mu = [e[a] + S[a] / (dn * s_fix) for a in range(dim)]
    # 1. the mean's image and its cell
    inside = np.ones(k.size, dtype=bool)
    within = np.ones(k.size, dtype=bool)                                    # ... the ring included
    j = []
    inv_c = np.float32(1.0 / cd)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(dim):
            p = (_row(Rm, r, mu, dim) + t[r]).astype(np.float32)
            f = (p - dorg[r]) * inv_c                                       # float32
            inside &= (f >= np.float32(ring)) & (f < np.float32(dext[r] - ring))
            within &= (f >= np.float32(0)) & (f < np.float32(dext[r]))
            j.append(np.where(inside, f, 0).astype(np.int64))
    cell = j[0] + dext[0] * (j[1] + (dext[1] * j[2] if dim == 3 else 0))
    cell = np.where(inside, cell, -1)
    # 2. offset and rotated sums
    a_, r_ = [], []
    for r in range(dim):
        re = _row(Rm, r, e, dim) + t[r]
        a_.append((re - centres(dorg[r], dext[r], cd)[j[r]]) * d_fix)
        r_.append(kk * _row(Rm, r, S, dim))
    M = [[None] * 3 for _ in range(3)]
    for p, (i, m) in enumerate(pairs):
        M[i][m] = M[m][i] = src_cells["ss"][k, p].astype(np.float64)
    zero = np.zeros(k.size)
    T = [[_row(Rm, r, [M[0][m], M[1][m], M[2][m] if dim == 3 else zero], dim) for m in range(dim)] for r in range(dim)]
    # 3. the contribution
    dS = np.zeros((k.size, dim), dtype=np.int64)
    dSS = np.zeros((k.size, len(pairs)), dtype=np.int64)
    for i in range(dim):                                                    # (a block that lands outside contributes nothing)
        dS[:, i] = np.rint(np.where(inside, dn * a_[i] + r_[i], 0.0)).astype(np.int64)
    for p, (i, m) in enumerate(pairs):
        q = kk2 * _row(Rm, m, [T[i][0], T[i][1], T[i][2] if dim == 3 else zero], dim)
        dSS[:, p] = np.rint(np.where(inside, (((dn * a_[i]) * a_[m] + a_[i] * r_[m]) + a_[m] * r_[i]) + q, 0.0)).astype(np.int64)
    raised = np.zeros((k.size, dim), dtype=np.int64)
    if clamp:
        for i in range(dim):
            p = pairs.index((i, i))
            for q in np.flatnonzero(inside):
                nn, s, ss = int(n[q]), int(dS[q, i]), int(dSS[q, p])
                if nn * ss < s * s:
                    up = -((-s * s) // nn)                                  # ceil(s^2 / n)
                    raised[q, i] = up - ss
                    dSS[q, p] = up
    return dict(k=k, n=n, cell=cell, on_ring=within & ~inside, dS=dS, dSS=dSS, raised=raised, e=np.stack(e, 1), S_int=src_cells["s"][k],
                SS_int=src_cells["ss"][k], R=Rm, t=t, pairs=pairs)


def map_merge_ref(dst_blob, src_blob, pose, sign=1, clamp=True):
    """save_map(dst), save_map(src), pose, +1 (merge) or -1 (unmerge) -> (save_map(dst) afterwards, n_outside).  Sums are
    integers mod 2^64 and counts mod 2^32, as on the device."""
    hd, dcells = R.parse(dst_blob)
    hs, scells = R.parse(src_blob)
    if not all(math.isfinite(float(v)) for v in pose):
        raise MergeError("the pose is not finite")
    c = contributions(hs, scells, hd, pose, clamp)
    out = dcells.copy()
    inn = c["cell"] >= 0
    cell = c["cell"][inn]
    op = np.add.at if sign > 0 else np.subtract.at
    with np.errstate(over="ignore"):
        op(out["n"], cell, c["n"][inn].astype(np.uint32))
        for a in range(c["dS"].shape[1]):
            op(out["s"][:, a], cell, c["dS"][inn, a])
        for p in range(c["dSS"].shape[1]):
            op(out["ss"][:, p], cell, c["dSS"][inn, p])
    g = dict(hd)
    filed = int(c["n"][inn].sum())
    if hd["dims"] == 2:
        g["n_points"] = hd["n_points"] + (filed if sign > 0 else -filed)
    return R.pack(g, out), int(c["n"][~inn].sum())


def clamp_acted(dst_blob, src_blob, pose):
    """Does the merge raise some diagonal second sum?"""
    hd, _ = R.parse(dst_blob)
    hs, scells = R.parse(src_blob)
    c = contributions(hs, scells, hd, pose)
    return bool(np.any(c["raised"][c["cell"] >= 0] > 0))


# ---- how far a contribution may lie from its exact value ---------------------------------------------------------------
U = Fr(1, 2 ** 53)          # unit roundoff of float64
G = (1 + U) ** 16 - 1       # a chain of at most 16 rounded operations


def exact_contribution(c, q, hs, hd):
    """Contribution q of `c` (contributions(), filed) without rounding, and how far the integers may lie from it.

    Exact value: X_a = n a_a + r_a and XX_ab = n a_a a_b + a_a r_b + a_b r_a + Q_ab with a = ((R e + t) - centre) fd,
    r = k (R S), Q = k^2 (R SS R^T) evaluated in rationals from the float64 inputs (R, t, the cell centres, fd, k) and the
    integer sums.  Expanding sum (R (e + u k / fd) + t - centre) fd over the source cell's quantised points u shows that
    these are, exactly, the first and second raw moments about the destination cell's centre, in dst units, of those points
    moved by p -> R p + t.

    Bound: the integer is rint(fl(expr)), so |integer - expr| <= 1/2 + |fl(expr) - expr|.
      * r and Q are sums of products of inputs; every term passes through at most 16 rounded operations on its way into the
        final sum (the deepest, an entry of Q: int64 -> double, a product and two sums for R SS, a product and two sums for
        (.) R^T, the product with k^2, three sums of the outer expression, and k^2 = fl(k k) itself), so standard forward error
        analysis bounds their share by G x the sum of the magnitudes of the terms, G = (1 + u)^16 - 1.
      * a is a DIFFERENCE of numbers of the map's size, so its error is absolute, not relative: fl(a) - a is at most
        da_r = G (sum_i |R_ri e_i| + |t_r| + |centre_r|) fd.  It enters X_a as n da_a and XX_ab as
        da_a (n |a_b| + |r|_b) + da_b (n |a_a| + |r|_a) + n da_a da_b, where |r|_a = k sum_i |R_ai S_i|.
    Returns (X [dim], XX [npair], B1 [dim], B2 [npair]) as Fractions, B = the bounds with the 1/2 included (before the
    clamp; a raised diagonal sum lies above by c["raised"])."""
    dim, sext, sorg, cs = _geometry(hs)
    _, dext, dorg, cd = _geometry(hd)
    Rm = [[Fr(v) for v in row] for row in c["R"]]
    t = [Fr(v) for v in c["t"]]
    e = [Fr(float(v)) for v in c["e"][q]]
    fd, kk = Fr(FIX / cd), Fr(cs / cd)
    cell = int(c["cell"][q])
    jd = [cell % dext[0], (cell // dext[0]) % dext[1]] + ([cell // (dext[0] * dext[1])] if dim == 3 else [])
    cen = [Fr(float(centres(dorg[a], dext[a], cd)[jd[a]])) for a in range(dim)]
    S = [Fr(int(v)) for v in c["S_int"][q]]
    SS = [[None] * dim for _ in range(dim)]
    for p, (i, m) in enumerate(c["pairs"]):
        SS[i][m] = SS[m][i] = Fr(int(c["SS_int"][q][p]))
    n = Fr(int(c["n"][q]))
    a = [(sum(Rm[r][i] * e[i] for i in range(dim)) + t[r] - cen[r]) * fd for r in range(dim)]
    da = [G * (sum(abs(Rm[r][i] * e[i]) for i in range(dim)) + abs(t[r]) + abs(cen[r])) * fd for r in range(dim)]
    r_ = [kk * sum(Rm[r][i] * S[i] for i in range(dim)) for r in range(dim)]
    rabs = [kk * sum(abs(Rm[r][i] * S[i]) for i in range(dim)) for r in range(dim)]
    X = [n * a[i] + r_[i] for i in range(dim)]
    B1 = [Fr(1, 2) + G * (abs(n * a[i]) + rabs[i]) + n * da[i] for i in range(dim)]
    XX, B2 = [], []
    for (i, m) in c["pairs"]:
        Qe = kk * kk * sum(Rm[i][u] * SS[u][v] * Rm[m][v] for u in range(dim) for v in range(dim))
        Qa = kk * kk * sum(abs(Rm[i][u] * SS[u][v] * Rm[m][v]) for u in range(dim) for v in range(dim))
        XX.append(n * a[i] * a[m] + a[i] * r_[m] + a[m] * r_[i] + Qe)
        mag = abs(n * a[i] * a[m]) + abs(a[i]) * rabs[m] + abs(a[m]) * rabs[i] + Qa
        B2.append(Fr(1, 2) + G * mag + da[i] * (n * abs(a[m]) + rabs[m]) + da[m] * (n * abs(a[i]) + rabs[i]) + n * da[i] * da[m])
    return X, XX, B1, B2


# ---- an oracle grid from a blob's sums ----------------------------------------------------------------------------------
def grid_from_blob(blob, prm):
    """oracle.ndt2d.Grid2D of a 2D blob: mean = centre + S / (n fs), M2 = (n SS - S S^T) / (n fs^2) from the exact integers,
    then oracle.ndt2d.finalise_cell - what ndt2d_load_map derives, in float64."""
    from oracle import ndt2d as O
    h, cells = R.parse(blob)
    assert h["dims"] == 2 and h["ngrid"] == 1
    W, H, c = h["width"], h["height"], float(h["cell_size"])
    ox, oy = np.float32(h["origin"][0][0]), np.float32(h["origin"][0][1])
    fs = FIX / c
    nc = W * H
    mean, icov, valid = np.zeros((nc, 2)), np.zeros((nc, 3)), np.zeros(nc, dtype=bool)
    cx, cy = centres(ox, W, c), centres(oy, H, c)
    count = cells["n"][:nc].astype(np.int64)
    for k in np.flatnonzero(count >= max(prm.min_points, 2)):
        n = int(count[k])
        s = [int(v) for v in cells["s"][k]]
        ss = [int(v) for v in cells["ss"][k]]
        mx, my = cx[k % W] + s[0] / (n * fs), cy[k // W] + s[1] / (n * fs)
        den = n * fs * fs
        m2 = [(n * ss[0] - s[0] * s[0]) / den, (n * ss[1] - s[0] * s[1]) / den, (n * ss[2] - s[1] * s[1]) / den]
        ok, a, b, cc = O.finalise_cell(n, mx, my, m2[0], m2[1], m2[2], prm)
        if ok:
            valid[k], mean[k], icov[k] = True, (mx, my), (a, b, cc)
    return O.Grid2D(ox, oy, np.float32(1.0 / c), W, H, count, mean, icov, valid, int(valid.sum()))
