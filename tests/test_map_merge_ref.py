"""The restatement of ndt*_merge_map / ndt*_unmerge_map (tests/map_merge_ref.py, docs/ALGORITHM.md section 2.18) checked
against what it must be, on the CPU and without the code under test: a whole-cell shift reproduces a build from the shifted
points byte for byte; at a general pose counts are conserved and every contribution - hence the merged map's global moments
- lies within a derived bound of the moments of the transformed points; unmerge inverts merge and merges commute; every
merged cell is one ndt*_load_map accepts; and a map merged from two halves localises a scan nearly as well as a map built
from the points of both."""
import math
from fractions import Fraction as Fr

import numpy as np
import pytest

import coarsen_cases as K
import map_coarsen_ref as R
import map_merge_ref as M
import merge_cases as MC


def _src_blob(dim, scene="tiny"):
    pts = MC.points(dim, scene)
    return pts, R.blob_from_points(pts, MC.C2 if dim == 2 else MC.C3)[0]


def _dst_blob(dim, scene="tiny", margin=2.0, own=True, c=None):
    c = c or (MC.C2 if dim == 2 else MC.C3)
    lo, hi = MC.extent(dim, scene, margin)
    origin, ext = MC.reserved_geometry(dim, lo, hi, c)
    pts = MC.own_points(dim, scene) if own else np.zeros((0, dim), dtype=np.float32)
    return R.blob_from_points(pts, c, origin, ext)[0]


@pytest.mark.parametrize("dim", [2, 3])
def test_whole_cell_shift_equals_a_build_from_the_shifted_points(dim):
    """pose = whole cells, equal cell sizes, coordinates on the 2^-11 lattice with fewer than 2048 points per cell: every
    double product is exact, so the merge into an empty reserved grid is the blob of the shifted points."""
    c = MC.C2 if dim == 2 else MC.C3
    k0, ext, n = (MC.SCENES2 if dim == 2 else MC.SCENES3)["tiny"]
    pts = K.lattice_cloud(17, k0, ext, c, n)
    src = R.blob_from_points(pts, c)[0]
    assert R.parse(src)[1]["n"].max() < 2048
    shift = np.array([3 * c, -2 * c, c][:dim])
    pose = tuple(shift) + (0.0,) * (1 if dim == 2 else 3 + 3 - dim)
    moved = (pts.astype(np.float64) + shift).astype(np.float32)
    assert np.array_equal(moved.astype(np.float64), pts.astype(np.float64) + shift)
    lo, hi = moved.min(axis=0) - 2 * c, moved.max(axis=0) + 2 * c
    origin, dext = MC.reserved_geometry(dim, lo, hi, c)
    got, outside = M.map_merge_ref(MC.empty_blob(dim, c, origin, dext), src, pose)
    want = R.blob_from_points(moved, c, origin, dext)[0]
    assert outside == 0
    assert np.array_equal(got, want)


def _world_moments_of_points(c, q_list, hs, hd, pts, dim):
    """Exact global first and second moments, in dst units about the world origin, of the source's quantised points moved by
    p -> R p + t, over the source cells q_list (those that were filed)."""
    _, sext, sorg, cs = M._geometry(hs)
    cd = float(hd["cell_size"])
    idx, Uq = MC.fixed_units(pts, cs, sorg)
    key = idx[:, 0] + sext[0] * (idx[:, 1] + (sext[1] * idx[:, 2] if dim == 3 else 0))
    filed = set(int(c["k"][q]) for q in q_list)
    Rm = [[Fr(v) for v in row] for row in c["R"]]
    t = [Fr(v) for v in c["t"]]
    fd, fs = Fr(M.FIX / cd), Fr(M.FIX / cs)
    cen = [M.centres(sorg[a], sext[a], cs) for a in range(dim)]
    G1 = [Fr(0)] * dim
    G2 = [Fr(0)] * len(c["pairs"])
    for i in range(len(pts)):
        if int(key[i]) not in filed:
            continue
        p = [Fr(float(cen[a][idx[i, a]])) + Fr(int(Uq[i, a])) / fs for a in range(dim)]
        w = [(sum(Rm[r][a] * p[a] for a in range(dim)) + t[r]) * fd for r in range(dim)]
        G1 = [G1[a] + w[a] for a in range(dim)]
        G2 = [G2[j] + w[a] * w[b] for j, (a, b) in enumerate(c["pairs"])]
    return G1, G2


@pytest.mark.parametrize("dim", [2, 3])
def test_counts_and_moments_are_conserved_at_a_general_pose(dim):
    """Total n + n_outside = the source's total.  Per contribution q the integers lie within exact_contribution's bound of
    the exact moments of the moved points about the destination cell's centre C_q (plus what the clamp raised).  Moving the
    reference point from C_q to the world origin gives, for the merged map's global moments G (sum over cells of
    n C + S and n C_a C_b + C_a S_b + C_b S_a + SS_ab, exact integers and rationals) against those of the moved points,
        |dG1_a|  <= sum_q B1_qa
        |dG2_ab| <= sum_q (B2_qab + |C_qa| B1_qb + |C_qb| B1_qa + raised_q [a = b]),
    which is what is asserted.  B1, B2 are 1/2 plus a float64 evaluation term: below 2^-10 for the first sums (asserted),
    and for the second sums - which reach 2^49 here, where 16 roundings of 2^-53 each are one unit - of the order of a unit
    (the largest is printed).  So this is the issue's "half a unit per contribution plus the clamp's raises" with the
    evaluation error of the float64 formula written out instead of ignored."""
    _counts_and_moments_are_conserved(dim, "general")


@pytest.mark.parametrize("pose_name", MC.TILTED)
def test_counts_and_moments_are_conserved_at_tilted_poses(pose_name):
    """The same at roll and pitch of 0.5 rad and more, in 3D."""
    _counts_and_moments_are_conserved(3, pose_name)


def _counts_and_moments_are_conserved(dim, pose_name):
    pts, src = _src_blob(dim)
    dst0 = _dst_blob(dim, own=False)
    pose = MC.poses(dim, "tiny")[pose_name]
    merged, outside = M.map_merge_ref(dst0, src, pose)
    hs, scells = R.parse(src)
    hd, mcells = R.parse(merged)
    assert int(mcells["n"].sum()) + outside == int(scells["n"].sum()) == len(pts)
    if dim == 2:
        assert hd["n_points"] == len(pts) - outside
    c = M.contributions(hs, scells, hd, pose)
    filed = [q for q in range(c["k"].size) if c["cell"][q] >= 0]
    assert len(filed) > 20 and np.any(c["raised"] > 0)
    _, dext, dorg, cd = M._geometry(hd)
    fd = Fr(M.FIX / cd)
    cen = [M.centres(dorg[a], dext[a], cd) for a in range(dim)]
    pairs = c["pairs"]
    tol1, tol2 = [Fr(0)] * dim, [Fr(0)] * len(pairs)
    worst_b2 = Fr(0)
    for q in filed:
        X, XX, B1, B2 = M.exact_contribution(c, q, hs, hd)
        cell = int(c["cell"][q])
        jd = [cell % dext[0], (cell // dext[0]) % dext[1]] + ([cell // (dext[0] * dext[1])] if dim == 3 else [])
        C = [Fr(float(cen[a][jd[a]])) * fd for a in range(dim)]
        for a in range(dim):
            assert abs(int(c["dS"][q, a]) - X[a]) <= B1[a] < Fr(1, 2) + Fr(1, 1024)
            tol1[a] += B1[a]
        for j, (a, b) in enumerate(pairs):
            up = int(c["raised"][q, a]) if a == b else 0
            assert abs(int(c["dSS"][q, j]) - up - XX[j]) <= B2[j]
            worst_b2 = max(worst_b2, B2[j])
            tol2[j] += B2[j] + abs(C[a]) * B1[b] + abs(C[b]) * B1[a] + up
    # the merged map's global moments
    G1, G2 = [Fr(0)] * dim, [Fr(0)] * len(pairs)
    for k in np.flatnonzero(mcells["n"]):
        k = int(k)
        jd = [k % dext[0], (k // dext[0]) % dext[1]] + ([k // (dext[0] * dext[1])] if dim == 3 else [])
        C = [Fr(float(cen[a][jd[a]])) * fd for a in range(dim)]
        n = int(mcells["n"][k])
        S = [int(v) for v in mcells["s"][k]]
        for a in range(dim):
            G1[a] += n * C[a] + S[a]
        for j, (a, b) in enumerate(pairs):
            G2[j] += n * C[a] * C[b] + C[a] * S[b] + C[b] * S[a] + int(mcells["ss"][k][j])
    P1, P2 = _world_moments_of_points(c, filed, hs, hd, pts, dim)
    for a in range(dim):
        assert abs(G1[a] - P1[a]) <= tol1[a]
    for j in range(len(pairs)):
        assert abs(G2[j] - P2[j]) <= tol2[j]
    print(f"dim {dim}: {len(filed)} contributions, {int((c['raised'] > 0).sum())} raised; |dG1| "
          f"{[float(abs(G1[a] - P1[a])) for a in range(dim)]} of {[float(v) for v in tol1]}; largest second-sum bound {float(worst_b2):.3f}")


@pytest.mark.parametrize("dim", [2, 3])
def test_unmerge_inverts_and_merges_commute(dim):
    _unmerge_inverts_and_merges_commute(dim, "general", "near_pi")


def test_unmerge_inverts_and_merges_commute_at_tilted_poses():
    _unmerge_inverts_and_merges_commute(3, "steep", "near_gimbal")


def _unmerge_inverts_and_merges_commute(dim, name_b, name_c):
    pts, b = _src_blob(dim)
    c_blob = R.blob_from_points(MC.points(dim, "tiny", seed=29), MC.C2 if dim == 2 else MC.C3)[0]
    a = _dst_blob(dim)
    P = MC.poses(dim, "tiny")
    tb, tc = P[name_b], P[name_c]
    ab, out_b = M.map_merge_ref(a, b, tb)
    assert not np.array_equal(ab, a)
    back, out_b2 = M.map_merge_ref(ab, b, tb, sign=-1)
    assert out_b2 == out_b and np.array_equal(back, a)
    abc = M.map_merge_ref(ab, c_blob, tc)[0]
    acb = M.map_merge_ref(M.map_merge_ref(a, c_blob, tc)[0], b, tb)[0]
    assert np.array_equal(abc, acb)
    # unmerge is the inverse whatever happened in between
    assert np.array_equal(M.map_merge_ref(abc, b, tb, sign=-1)[0], M.map_merge_ref(a, c_blob, tc)[0])


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("half", [False, True])
def test_every_merged_cell_is_one_load_map_accepts(dim, half):
    """With the clamp every contribution is a plausible cell on its own, and by Cauchy-Schwarz so is every sum of them;
    without it some contribution of the tiny scene is not (n dSS_aa < dS_a^2: the clamp is needed)."""
    pts, src = _src_blob(dim)
    c_d = (MC.C2 if dim == 2 else MC.C3) * (2 if half else 1)
    dst0 = _dst_blob(dim, own=False, c=c_d)
    hs, scells = R.parse(src)
    diag = [j for j, (a, b) in enumerate(M.pairs_of(dim)) if a == b]
    off = [j for j in range(len(M.pairs_of(dim))) if j not in diag]

    def plausible(n, s, ss):
        return R.cell_sums_plausible(int(n), [int(v) for v in s], [int(ss[j]) for j in diag], [int(ss[j]) for j in off])

    needed = 0
    for name, pose in MC.poses(dim, "tiny").items():
        cells = R.parse(M.map_merge_ref(dst0, src, pose)[0])[1]
        for k in np.flatnonzero(cells["n"]):
            assert plausible(cells["n"][k], cells["s"][k], cells["ss"][k]), (name, k)
        raw = M.contributions(hs, scells, R.parse(dst0)[0], pose, clamp=False)
        needed += sum(not plausible(raw["n"][q], raw["dS"][q], raw["dSS"][q]) for q in np.flatnonzero(raw["cell"] >= 0))
    assert needed > 0


def _rms(points, est, truth):
    def move(p):
        c, s = math.cos(p[2]), math.sin(p[2])
        return np.stack([c * points[:, 0] - s * points[:, 1] + p[0], s * points[:, 0] + c * points[:, 1] + p[1]], 1)
    return float(np.sqrt(np.mean(np.sum((move(est) - move(truth)) ** 2, axis=1))))


def test_a_merged_map_localises_nearly_as_well_as_a_map_of_the_points():
    """Two halves A and B of one synth config-2 scene (a 50 m room), B in its own frame T_B; merged = merge(A, B, T_B) and
    direct = a build from A and T_B B together, both on one reserved lattice.  A third cloud C of the same room is aligned
    map-to-map (tests/d2d_ref.py, float64) against both from the same offset start, and the error against the pose that
    generated C - the RMS distance between C's points under the estimated and the true pose - may be at most twice the
    direct map's own: what a map is allowed to lose by replacing each source cell's points by two moments filed as a block.
    Measured: see the printed line (recorded in DESIGN section 5.15)."""
    import d2d_ref as D
    from gtsam_ndt_amd import synth
    from oracle import ndt2d as O
    d = synth.make_pair(2)
    c = d["cell"]
    world = np.stack([d["tx"], d["ty"]], 1).astype(np.float64)
    left = world[:, 0] < 2.0
    A = world[left].astype(np.float32)
    tb = (3.7, -2.2, 0.4)
    cs, sn = math.cos(tb[2]), math.sin(tb[2])
    bw = world[~left] - np.array(tb[:2])
    B = np.stack([cs * bw[:, 0] + sn * bw[:, 1], -sn * bw[:, 0] + cs * bw[:, 1]], 1).astype(np.float32)       # T_B^-1 world
    Bw = np.stack([cs * B[:, 0].astype(np.float64) - sn * B[:, 1] + tb[0], sn * B[:, 0].astype(np.float64) + cs * B[:, 1] + tb[1]], 1).astype(np.float32)
    origin, ext = MC.reserved_geometry(2, world.min(axis=0) - 1.0, world.max(axis=0) + 1.0, c)
    a_blob = R.blob_from_points(A, c, origin, ext)[0]
    merged, outside = M.map_merge_ref(a_blob, R.blob_from_points(B, c)[0], tb)
    direct = R.blob_from_points(np.vstack([A, Bw]), c, origin, ext)[0]
    assert outside == 0 and R.parse(merged)[0]["n_points"] == R.parse(direct)[0]["n_points"] == len(world)
    prm = O.NdtParams(cell_size=c)
    comps = D.build_map(d["sx"], d["sy"], prm)[1]
    start = (d["init"][0] + 0.25, d["init"][1] - 0.2, d["init"][2] + 0.02)
    src_pts = np.stack([d["sx"], d["sy"]], 1).astype(np.float64)
    err = {}
    for name, blob in (("merged", merged), ("direct", direct)):
        r = D.align(M.grid_from_blob(blob, prm), comps, start, prm)
        assert r["status"] == O.NDT_OK, (name, r["status"])
        err[name] = _rms(src_pts, r["pose"], d["pose"])
    print(f"quality: RMS error against the truth, merged map {err['merged']:.3e} m, direct map {err['direct']:.3e} m "
          f"(ratio {err['merged'] / err['direct']:.2f})")
    assert err["merged"] <= 2.0 * err["direct"]
