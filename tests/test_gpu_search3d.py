"""Exhaustive 3D pose search (ndt3d_search_*): a relocalisation the local optimiser cannot do, the score volume against
the oracle, the hits against the numpy restatement in gtsam_ndt_amd/search.py, the composition with the multi-start
chain, determinism, and the edges."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import search, synth3d

pytestmark = pytest.mark.gpu

DEG = math.pi / 180.0
GOLD3 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ndt3d_small.npz")


def _dev(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in arrays)


def _same(a, b):
    return (a.pose == b.pose and a.iterations == b.iterations and a.status == b.status and a.n_hit == b.n_hit
            and a.score == b.score and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g))


def _dist(p, q):
    """translation (x, y, z) and rotation (largest of the wrapped roll, pitch, yaw differences) between two poses"""
    dt = math.sqrt(sum((p[a] - q[a]) ** 2 for a in range(3)))
    dr = max(abs(float(search.wrap(p[a] - q[a]))) for a in range(3, 6))
    return dt, dr


@pytest.fixture(scope="module")
def small():
    g = np.load(GOLD3)
    return {k: np.ascontiguousarray(g[k], dtype=np.float32) for k in ("tx", "ty", "tz", "sx", "sy", "sz")} | {
        "init": tuple(float(v) for v in g["init"]), "pose": tuple(float(v) for v in g["final_pose"])}


@pytest.fixture(scope="module")
def relocal():
    """The 40 m box room: target = a 64 x 1024 scan from the origin, source = a 32 x 512 scan from P."""
    zero = (0.0,) * 6
    t = synth3d.lidar_scan(101, zero, 64, 1024).astype(np.float32)
    s = synth3d.lidar_scan(102, RELOCAL_P, 32, 512).astype(np.float32)
    return {"t": [np.ascontiguousarray(t[:, a]) for a in range(3)], "s": [np.ascontiguousarray(s[:, a]) for a in range(3)]}


RELOCAL_P = (3.0, -2.5, 0.0, 0.006, -0.005, 1.2)
RELOCAL_GUESS = (RELOCAL_P[0] + 1.5, RELOCAL_P[1] - 1.25, 0.0, 0.0, 0.0, RELOCAL_P[5] + 0.8)


def test_search_recovers_a_pose_local_alignment_cannot(gpu_lib, relocal):
    """The scene of the issue with a smaller roll and pitch (0.006, -0.005: within its 0.02 rad), every 8th point of the
    scan, +-3 m x +-3 m x a full turn at 0.25 m / 1 degree, k = 8.
    Checked with the oracle on the CPU first (every 8th point, roll = pitch = 0 pinned): the lattice pose nearest P,
    (3.0, -2.5, yaw 1.1971), scores 126.6, its 26 lattice neighbours at most 113.8 and 1500 random lattice poses of the
    window at most 109.9: it is a peak.  Of the 26 poses 0.5 m / 4 degrees away one outscores it: (3.0, -2.0) with 141.3,
    which refines to a non-converged pose 0.6 m from P.  A finer subsample does not change that: with the issue's
    roll = 0.02, pitch = -0.015 the figures are 92.6 (nearest), 115.3 (a neighbour), 132.2 (0.5 m away) for every 8th
    point and 750 / 930 / 1001 for the full scan, the same ratios.  So the assertion is the issue's, on the refined
    result: the search returns 8 separated hits and the refinement on the full scan picks the one in P's basin (on the
    MI355X the second hit, lattice scores 141.302 and 126.558 as the oracle's)."""
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    from oracle import ndt3d as o
    P, guess = RELOCAL_P, RELOCAL_GUESS
    t, s = relocal["t"], relocal["s"]
    full = _dev(*s)
    sub = _dev(*(a[::8] for a in s))
    with NdtMatcher3D() as m:
        m.set_target(*t)
        # the premise: neither the local optimiser nor a small multi-start lattice reaches P from the guess
        r = m.align(*full, guess)
        print("align from the guess:", r.pose, r.status, _dist(r.pose, P))
        assert _dist(r.pose, P)[0] > 0.2
        starts = [(guess[0] + a, guess[1] + b, 0.0, 0.0, 0.0, guess[5] + c) for a in np.linspace(-0.3, 0.3, 4)
                  for b in np.linspace(-0.3, 0.3, 4) for c in np.linspace(-0.1, 0.1, 4)]
        multi = m.align_multi_start(*full, starts)
        best_multi = max((q for q in multi if q.status == L.NDT_OK), key=lambda q: q.score, default=None)
        print("best of 64 starts around the guess:", best_multi and (best_multi.pose, _dist(best_multi.pose, P)))
        assert best_multi is None or _dist(best_multi.pose, P)[0] > 0.2
        center = (guess[0], guess[1], 0.0, 0.0, 0.0, guess[5])
        hits = m.search(*sub, center, (3.0, 3.0, math.pi), (0.25, 0.25, DEG), k=8)
        assert hits
        for h in hits:
            print("hit", h)
        refined = m.align_multi_start(*full, [h.pose for h in hits])
    hit, best = max(((h, q) for h, q in zip(hits, refined) if q.status == L.NDT_OK), key=lambda hq: hq[1].score)
    dt, dr = _dist(best.pose, P)
    print("best refined:", best.pose, "from", hit, "distance", dt, dr)
    assert dt < 0.02 and dr < 0.005, (best.pose, P)
    prm = o.Ndt3Params()
    ref = o.align3(o.build_grid3(*t, prm), *s, hit.pose, prm)
    assert np.max(np.abs(np.array(best.pose) - np.array(ref["pose"]))) < 1e-4


def test_score_volume_matches_the_oracle(gpu_lib, small):
    """The golden pair, a window of 9 x 9 x 36 = 2916 poses with a non-zero pinned z, roll and pitch.  Reference:
    oracle.ndt3d.evaluate3(mirror32=True) at every lattice pose."""
    d = small
    c = (d["pose"][0] + 0.05, d["pose"][1] - 0.05, 0.04, 0.012, -0.008, d["pose"][5])
    _score_volume_matches_the_oracle(d, search.Window(c, (0.8, 0.8, math.pi), (0.2, 0.2, 10.0 * DEG)), (36, 9, 9))


def test_score_volume_matches_the_oracle_at_a_steep_pinned_roll_and_pitch(gpu_lib, small):
    """The same with roll 0.7 and pitch -0.5 pinned: the golden source seen from a frame tilted that far
    (tilted_cases.tilted_pair), 5 x 5 x 9 = 225 poses round the pose that puts it back onto the target."""
    import tilted_cases as T
    t = T.tilted_pair("steep")
    d = dict(small, sx=t["sx"], sy=t["sy"], sz=t["sz"])
    c = (d["pose"][0] + 0.05, d["pose"][1] - 0.05, 0.04, 0.7, -0.5, 2.1)
    _score_volume_matches_the_oracle(d, search.Window(c, (0.4, 0.4, 40.0 * DEG), (0.2, 0.2, 10.0 * DEG)), (9, 5, 5))


def _score_volume_matches_the_oracle(d, window, dims):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    from oracle import ndt3d as o
    c = window[0]
    assert search.dims(window)[0] == dims
    prm = o.Ndt3Params()
    g = o.build_grid3(d["tx"], d["ty"], d["tz"], prm)
    xs, ys, th = search.lattice(window)
    ref = np.zeros((th.size, ys.size, xs.size))
    for j, yaw in enumerate(th):
        for iy, y in enumerate(ys):
            for ix, x in enumerate(xs):
                ref[j, iy, ix] = o.evaluate3(g, d["sx"], d["sy"], d["sz"], (x, y, c[2], c[3], c[4], yaw), prm, mirror32=True)[2]
    s = _dev(d["sx"], d["sy"], d["sz"])
    with NdtMatcher3D() as m:
        m.set_target(d["tx"], d["ty"], d["tz"])
        vol = m.search_scores(*s, *window).cpu().numpy().astype(np.float64)
        hits = m.search(*s, *window, k=8)
        assert hits
        for h in hits:
            assert h.pose[2:5] == c[2:5]
            ev = m.evaluate(*s, h.pose)[2]
            print("hit", h, "evaluate", ev, "relative difference", abs(h.score - ev) / abs(ev))
            assert abs(h.score - ev) <= 1e-5 * abs(ev), (h, ev)
    assert vol.shape == ref.shape
    err = np.abs(vol - ref)
    print("volume against the oracle: max |err|", float(err.max()), "max |err| / |ref|", float(np.max(err / np.maximum(np.abs(ref), 1e-30))),
          "max (|err| - 1e-4 |ref|)", float(np.max(err - 1e-4 * np.abs(ref))), "max ref", float(ref.max()))
    assert np.all(err <= 1e-4 * np.abs(ref) + 1e-3), float(np.max(err - 1e-4 * np.abs(ref)))
    assert np.max(ref) > 10.0           # the window holds the true pose: a real peak, not an empty map


@pytest.mark.parametrize("case", ["cyclic", "window", "ties", "sparse"])
def test_hits_are_exactly_the_specification(gpu_lib, small, case):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = small
    p = d["pose"]
    c = (p[0], p[1], 0.02, 0.01, -0.01, p[5])
    window, k, sep = {
        "cyclic": (search.Window(c, (1.0, 1.0, math.pi), (0.1, 0.1, 10.0 * DEG)), 16, (0.5, 0.1)),
        "window": (search.Window((c[0] + 0.1, c[1], 0.0, 0.0, 0.0, 0.2), (0.5, 0.4, 0.3), (0.05, 0.05, 0.05)), 12, (0.2, 0.05)),
        # most of this window lies outside the 40 m room: wide regions of score 0
        "ties": (search.Window((38.0, 0.0, 0.0, 0.0, 0.0, 0.0), (12.0, 4.0, 0.2), (1.0, 1.0, 0.1)), 64, (0.0, 0.0)),
        "sparse": (search.Window(c, (1.0, 1.0, math.pi), (0.1, 0.1, 10.0 * DEG)), 8, (100.0, 10.0)),
    }[case]
    s = _dev(d["sx"], d["sy"], d["sz"])
    with NdtMatcher3D() as m:
        m.set_target(d["tx"], d["ty"], d["tz"])
        vol = m.search_scores(*s, *window).cpu().numpy()
        got = m.search(*s, *window, k=k, min_sep=sep)
    want = search.select_hits(vol, window, k, sep)
    assert got == want
    assert got and all(len(h.pose) == 6 for h in got)
    if case == "ties":
        assert np.count_nonzero(vol == 0) > vol.size // 4
    if case == "sparse":
        assert len(got) == 1 < k


def test_composition_and_determinism(gpu_lib, small):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = small
    p = d["pose"]
    window = search.Window((p[0], p[1], 0.0, 0.0, 0.0, p[5]), (1.0, 1.0, math.pi), (0.1, 0.1, 10.0 * DEG))
    s = _dev(d["sx"], d["sy"], d["sz"])
    with NdtMatcher3D() as m:
        m.set_target(d["tx"], d["ty"], d["tz"])
        out = m.search_align(*s, *window, k=6)
        assert len(out) == 6
        multi = m.align_multi_start(*s, [h.pose for h, _ in out])
        for (h, r), q in zip(out, multi):
            assert _same(r, q), (r, q)
        v1 = m.search_scores(*s, *window)
        v2 = m.search_scores(*s, *window)
        assert np.array_equal(v1.cpu().numpy().view(np.uint32), v2.cpu().numpy().view(np.uint32))
        h1 = m.search(*s, *window, k=8)
        h2 = m.search(*s, *window, k=8)
        h_host = m.search(d["sx"], d["sy"], d["sz"], *window, k=8)
        assert h1 == h2 == h_host
        assert [h for h, _ in out] == h1[:6]


def _window(center, half, step, sep=(0.5, 0.1)):
    w = L.SearchWindow3D()
    for a in range(6):
        w.center[a] = center[a]
    for a in range(3):
        w.half_extent[a], w.step[a] = half[a], step[a]
    w.min_sep_trans, w.min_sep_rot = sep
    return w


def test_edges_and_errors_leave_the_handle_intact(gpu_lib, small):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = small
    lib = gpu_lib
    sx, sy, sz = _dev(d["sx"], d["sy"], d["sz"])
    n = sx.numel()
    ps = [C.c_void_p(a.data_ptr()) for a in (sx, sy, sz)]
    hits = (L.SearchHit3D * 64)()
    nh = C.c_int32(-1)
    c = d["pose"]
    good = _window(c, (0.5, 0.5, 0.2), (0.1, 0.1, 0.1))

    def run(m, w, k=8, hp=hits, ptrs=ps):
        return lib.ndt3d_search_dev(m._h, *ptrs, n, C.byref(w) if w is not None else None, k,
                                    C.cast(hp, C.c_void_p) if hp is not None else None, C.byref(nh))

    def nan_at(a):
        v = list(c)
        v[a] = math.nan
        return _window(v, (0.5, 0.5, 0.2), (0.1, 0.1, 0.1))

    with NdtMatcher3D() as fresh:
        assert run(fresh, good) == L.NDT_ERR_NO_TARGET
        fresh.set_target(d["tx"], d["ty"], d["tz"])
        ref1 = fresh.align(sx, sy, sz, d["init"])
    with NdtMatcher3D() as m:
        m.set_target(d["tx"], d["ty"], d["tz"])
        # a window far from the map: OK and no hits
        assert run(m, _window((500.0, 500.0, 0.0, 0.0, 0.0, 0.0), (1.0, 1.0, math.pi), (0.1, 0.1, 0.1))) == L.NDT_OK
        assert nh.value == 0
        bad = [_window(c, (0.5, 0.5, 0.2), (0.0, 0.1, 0.1)),
               _window(c, (-0.5, 0.5, 0.2), (0.1, 0.1, 0.1)),
               _window(c, (0.5, math.inf, 0.2), (0.1, 0.1, 0.1)),
               _window(c, (0.5, 0.5, 0.2), (0.1, 0.1, -0.1)),
               _window(c, (0.5, 0.5, 0.2), (0.1, 0.1, 0.1), (math.nan, 0.1)),
               _window(c, (0.5, 0.5, 0.2), (0.1, 0.1, 0.1), (0.1, -1.0))] + [nan_at(a) for a in range(6)]
        for w in bad:
            assert run(m, w) == L.NDT_ERR_INVALID_ARG
        assert run(m, good, k=0) == L.NDT_ERR_INVALID_ARG
        assert run(m, good, k=65) == L.NDT_ERR_INVALID_ARG
        assert run(m, None) == L.NDT_ERR_INVALID_ARG
        assert run(m, good, hp=None) == L.NDT_ERR_INVALID_ARG
        assert run(m, good, ptrs=[ps[0], ps[1], None]) == L.NDT_ERR_INVALID_ARG
        assert lib.ndt3d_search_dev(m._h, *ps, n, C.byref(good), 8, C.cast(hits, C.c_void_p), None) == L.NDT_ERR_INVALID_ARG
        assert lib.ndt3d_search_scores_dev(m._h, *ps, n, C.byref(good), None) == L.NDT_ERR_INVALID_ARG
        assert lib.ndt3d_search_align_dev(m._h, *ps, n, C.byref(good), 8, C.cast(hits, C.c_void_p), None,
                                          C.byref(nh)) == L.NDT_ERR_INVALID_ARG
        huge = _window((0.0,) * 6, (50.0, 50.0, math.pi), (0.01, 0.01, 0.1))
        assert run(m, huge) == L.NDT_ERR_CAPACITY
        dims = (C.c_int32 * 3)()
        assert lib.ndt3d_search_lattice_size(C.byref(huge), C.cast(dims, C.c_void_p)) == L.NDT_ERR_CAPACITY
        # after the errors the handle aligns as a fresh one does, bit for bit
        a1 = m.align(sx, sy, sz, d["init"])
        assert _same(a1, ref1)
        # a search between two alignments leaves the second one unchanged
        assert run(m, good) == L.NDT_OK and nh.value > 0
        a2 = m.align(sx, sy, sz, d["init"])
        assert _same(a2, ref1)
        # a search behind an alignment in flight finishes it first and does not disturb the next one
        m.align_async(sx, sy, sz, d["init"])
        assert run(m, good) == L.NDT_OK and nh.value > 0
        a3 = m.align(sx, sy, sz, d["init"])
        assert _same(a3, ref1)
