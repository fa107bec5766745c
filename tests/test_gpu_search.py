"""Exhaustive pose search (ndt2d_search_*): the score volume against the oracle, the hits against the numpy
restatement in gtsam_ndt_amd/search.py, the composition with the multi-start chain, determinism, and the edges."""
import ctypes as C
import math

import numpy as np
import pytest

from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import search, synth

pytestmark = pytest.mark.gpu

DEG = math.pi / 180.0


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def _same(a, b):
    return (a.pose == b.pose and a.iterations == b.iterations and a.status == b.status and a.n_hit == b.n_hit
            and a.score == b.score and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g))


@pytest.fixture(scope="module")
def pair1():
    return synth.make_pair(1)


@pytest.fixture(scope="module")
def relocal():
    """50 m room, 100k target points; a 1440-beam lidar scan from P (NaN returns kept)."""
    sc = synth.room_scene(4242, 50.0, -25.0, -25.0)
    tx, ty = synth.sample_scene(sc, 100_000, seed=4242 * 7919 + 11)
    P = (3.1, -4.2, 0.4)
    r, a0, inc = synth.lidar_scan2d(sc, P, n_beams=1440, seed=5)
    sx, sy = synth.scan_points(r, a0, inc)
    return {"tx": np.ascontiguousarray(tx, dtype=np.float32), "ty": np.ascontiguousarray(ty, dtype=np.float32),
            "sx": sx, "sy": sy, "P": P}


def _dist(p, q):
    return math.hypot(p[0] - q[0], p[1] - q[1]), abs(float(search.wrap(p[2] - q[2])))


def test_search_recovers_a_pose_local_alignment_cannot(gpu_lib, relocal):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    from oracle import ndt2d as o
    d = relocal
    P = d["P"]
    guess = (P[0] + 1.4, P[1] - 1.1, P[2] + 0.7)
    sx, sy = _dev(d["sx"]), _dev(d["sy"])
    with NdtMatcher2D() as m:
        m.set_target(d["tx"], d["ty"])
        # the premise: neither the local optimiser nor a small multi-start lattice reaches P from the guess
        r = m.align(sx, sy, guess)
        assert _dist(r.pose, P)[0] > 0.2
        starts = [(guess[0] + a, guess[1] + b, guess[2] + c) for a in np.linspace(-0.3, 0.3, 4)
                  for b in np.linspace(-0.3, 0.3, 4) for c in np.linspace(-0.1, 0.1, 4)]
        multi = m.align_multi_start(sx, sy, starts)
        best_multi = max((q for q in multi if q.converged), key=lambda q: q.score, default=None)
        assert best_multi is None or _dist(best_multi.pose, P)[0] > 0.2
        out = m.search_align(sx, sy, guess, (2.0, 2.0, math.pi), (0.1, 0.1, 2.0 * DEG), k=8)
    assert out
    hit, best = max(((h, q) for h, q in out if q.converged), key=lambda hq: hq[1].score)
    dt, dr = _dist(best.pose, P)
    assert dt < 0.02 and dr < 0.005, (best.pose, P)
    ok = np.isfinite(d["sx"]) & np.isfinite(d["sy"])
    prm = o.NdtParams()
    ref = o.align(o.build_grid(d["tx"], d["ty"], prm), d["sx"][ok], d["sy"][ok], hit.pose, prm)
    assert np.max(np.abs(np.array(best.pose) - np.array(ref["pose"]))) < 1e-4


def _oracle_volume(grids, sx, sy, window, prm):
    """The oracle's evaluation score at every lattice pose, vectorised per heading: float32 transform and cell keys as
    the device computes them (oracle mirror32), float64 terms and sums."""
    from oracle import ndt2d as o
    xs, ys, th = search.lattice(window)
    ok = np.isfinite(sx) & np.isfinite(sy)
    x, y = sx[ok].astype(np.float32), sy[ok].astype(np.float32)
    tx = xs.astype(np.float32)[None, :, None]
    ty = ys.astype(np.float32)[:, None, None]
    vol = np.zeros((th.size, ys.size, xs.size))
    for j, t in enumerate(th):
        c32, s32 = np.float32(math.cos(t)), np.float32(math.sin(t))
        # px = fmaf(c, x, fmaf(-s, y, tx)) over [y lattice, x lattice, points]
        inner_x = (y.astype(np.float64) * np.float64(-s32) + tx.astype(np.float64)).astype(np.float32)
        inner_y = (y.astype(np.float64) * np.float64(c32) + ty.astype(np.float64)).astype(np.float32)
        px = (x.astype(np.float64) * np.float64(c32) + inner_x.astype(np.float64)).astype(np.float32)
        py = (x.astype(np.float64) * np.float64(s32) + inner_y.astype(np.float64)).astype(np.float32)
        px, py = np.broadcast_arrays(px, py)
        for g in grids:
            key, inside = o.cell_keys32(px, py, g.ox, g.oy, g.inv_c, g.W, g.H)
            hit = inside & g.valid[key]
            qx = px.astype(np.float64) - g.mean[key, 0]
            qy = py.astype(np.float64) - g.mean[key, 1]
            a, b, cc = g.icov[key, 0], g.icov[key, 1], g.icov[key, 2]
            mm = qx * (a * qx + b * qy) + qy * (b * qx + cc * qy)
            with np.errstate(over="ignore", invalid="ignore"):
                s = np.where(hit, prm.d1 * np.exp(-0.5 * prm.d2 * np.where(hit, mm, 0.0)), 0.0)
            vol[j] += s.sum(axis=-1)
    return vol


@pytest.mark.parametrize("overlap", [1, 4])
def test_score_volume_matches_the_oracle(gpu_lib, pair1, overlap):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    from oracle import ndt2d as o
    d = pair1
    window = search.Window(d["init"], (1.0, 1.0, math.pi), (0.1, 0.1, 10.0 * DEG))
    assert search.dims(window)[0] == (36, 21, 21)
    prm = o.NdtParams(overlap=overlap)
    grids = o.build_grids(d["tx"], d["ty"], prm)
    ref = _oracle_volume(grids, d["sx"], d["sy"], window, prm)
    sx, sy = _dev(d["sx"]), _dev(d["sy"])
    with NdtMatcher2D(overlap_grids=overlap) as m:
        m.set_target(d["tx"], d["ty"])
        vol = m.search_scores(sx, sy, *window).cpu().numpy().astype(np.float64)
        hits = m.search(sx, sy, *window, k=8)
        assert hits
        for h in hits:
            ev = m.evaluate(sx, sy, h.pose)[2]
            assert abs(h.score - ev) <= 1e-5 * abs(ev), (h, ev)
    assert vol.shape == ref.shape
    err = np.abs(vol - ref)
    assert np.all(err <= 1e-4 * np.abs(ref) + 1e-3), float(np.max(err - 1e-4 * np.abs(ref)))
    assert np.max(ref) > 10.0           # the window holds the true pose: a real peak, not an empty map


@pytest.mark.parametrize("case", ["cyclic", "window", "ties", "sparse"])
def test_hits_are_exactly_the_specification(gpu_lib, pair1, case):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = pair1
    c = d["init"]
    window, k, sep = {
        "cyclic": (search.Window(c, (1.0, 1.0, math.pi), (0.1, 0.1, 10.0 * DEG)), 16, (0.5, 0.1)),
        "window": (search.Window((c[0] + 0.1, c[1], 0.2), (0.5, 0.4, 0.3), (0.05, 0.05, 0.05)), 12, (0.2, 0.05)),
        # most of this window lies outside the 8 m room: wide regions of score 0
        "ties": (search.Window((10.0, 0.0, 0.0), (3.0, 1.0, 0.2), (0.25, 0.25, 0.1)), 64, (0.0, 0.0)),
        "sparse": (search.Window(c, (1.0, 1.0, math.pi), (0.1, 0.1, 10.0 * DEG)), 8, (100.0, 10.0)),
    }[case]
    sx, sy = _dev(d["sx"]), _dev(d["sy"])
    with NdtMatcher2D() as m:
        m.set_target(d["tx"], d["ty"])
        vol = m.search_scores(sx, sy, *window).cpu().numpy()
        got = m.search(sx, sy, *window, k=k, min_sep=sep)
    want = search.select_hits(vol, window, k, sep)
    assert got == want
    if case == "ties":
        assert np.count_nonzero(vol == 0) > vol.size // 4
    if case == "sparse":
        assert len(got) == 1 < k


def test_composition_and_determinism(gpu_lib, pair1):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = pair1
    window = search.Window(d["init"], (1.0, 1.0, math.pi), (0.1, 0.1, 10.0 * DEG))
    sx, sy = _dev(d["sx"]), _dev(d["sy"])
    with NdtMatcher2D() as m:
        m.set_target(d["tx"], d["ty"])
        out = m.search_align(sx, sy, *window, k=6)
        assert len(out) == 6
        multi = m.align_multi_start(sx, sy, [h.pose for h, _ in out])
        for (h, r), q in zip(out, multi):
            assert _same(r, q), (r, q)
        v1 = m.search_scores(sx, sy, *window)
        v2 = m.search_scores(sx, sy, *window)
        assert np.array_equal(v1.cpu().numpy().view(np.uint32), v2.cpu().numpy().view(np.uint32))
        h1 = m.search(sx, sy, *window, k=8)
        h2 = m.search(sx, sy, *window, k=8)
        h_host = m.search(d["sx"], d["sy"], *window, k=8)
        assert h1 == h2 == h_host
        assert [h for h, _ in out] == h1[:6]


def _window(center, half, step, sep=(0.5, 0.1)):
    w = L.SearchWindow2D()
    for a in range(3):
        w.center[a], w.half_extent[a], w.step[a] = center[a], half[a], step[a]
    w.min_sep_trans, w.min_sep_rot = sep
    return w


def test_edges_and_errors_leave_the_handle_intact(gpu_lib, pair1):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = pair1
    lib = gpu_lib
    sx, sy = _dev(d["sx"]), _dev(d["sy"])
    n = sx.numel()
    ps, py_ = C.c_void_p(sx.data_ptr()), C.c_void_p(sy.data_ptr())
    hits = (L.SearchHit2D * 64)()
    nh = C.c_int32(-1)
    good = _window(d["init"], (0.5, 0.5, 0.2), (0.1, 0.1, 0.1))

    def run(m, w, k=8, hp=hits):
        return lib.ndt2d_search_dev(m._h, ps, py_, n, C.byref(w) if w is not None else None, k,
                                    C.cast(hp, C.c_void_p) if hp is not None else None, C.byref(nh))

    with NdtMatcher2D() as fresh:
        assert run(fresh, good) == L.NDT_ERR_NO_TARGET
        fresh.set_target(d["tx"], d["ty"])
        ref1 = fresh.align(sx, sy, d["init"])
    with NdtMatcher2D() as m:
        m.set_target(d["tx"], d["ty"])
        # a window far from the map: OK and no hits
        assert run(m, _window((500.0, 500.0, 0.0), (1.0, 1.0, math.pi), (0.1, 0.1, 0.1))) == L.NDT_OK
        assert nh.value == 0
        bad = [_window(d["init"], (0.5, 0.5, 0.2), (0.0, 0.1, 0.1)),
               _window(d["init"], (-0.5, 0.5, 0.2), (0.1, 0.1, 0.1)),
               _window((math.nan, 0.0, 0.0), (0.5, 0.5, 0.2), (0.1, 0.1, 0.1)),
               _window(d["init"], (0.5, math.inf, 0.2), (0.1, 0.1, 0.1)),
               _window(d["init"], (0.5, 0.5, 0.2), (0.1, 0.1, -0.1)),
               _window(d["init"], (0.5, 0.5, 0.2), (0.1, 0.1, 0.1), (math.nan, 0.1))]
        for w in bad:
            assert run(m, w) == L.NDT_ERR_INVALID_ARG
        assert run(m, good, k=0) == L.NDT_ERR_INVALID_ARG
        assert run(m, good, k=65) == L.NDT_ERR_INVALID_ARG
        assert run(m, None) == L.NDT_ERR_INVALID_ARG
        assert run(m, good, hp=None) == L.NDT_ERR_INVALID_ARG
        huge = _window((0.0, 0.0, 0.0), (50.0, 50.0, math.pi), (0.01, 0.01, 0.1))
        assert run(m, huge) == L.NDT_ERR_CAPACITY
        dims = (C.c_int32 * 3)()
        assert lib.ndt2d_search_lattice_size(C.byref(huge), C.cast(dims, C.c_void_p)) == L.NDT_ERR_CAPACITY
        # after the errors the handle aligns as a fresh one does, bit for bit
        a1 = m.align(sx, sy, d["init"])
        assert _same(a1, ref1)
        # a search between two alignments leaves the second one unchanged
        assert run(m, good) == L.NDT_OK and nh.value > 0
        a2 = m.align(sx, sy, d["init"])
        assert _same(a2, ref1)
