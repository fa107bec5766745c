"""Exhaustive pose search for map-to-map alignment on the device (ndt2d_search_map / ndt2d_search_map_scores /
ndt2d_search_align_map; docs/ALGORITHM.md section 2.15): the score volume against the float64 restatement
(tests/d2d_search_ref.py), the hits against the numpy specification (gtsam_ndt_amd/search.py), the composition with
ndt2d_align_map, determinism, the derived data following the grid, maps that never saw a point, and the error table.

Bounds.  Volume: |vol - ref| <= 1e-4 |ref| + 1e-3, the project's bound for a float32 private-sum score volume
(tests/test_gpu_search.py).  Hit scores: 1e-5 relative against ndt2d_evaluate_map (the same float32 terms in another
summation order).  Poses: 0.05 m / 0.005 rad of the generating pose (the centimetre-scale optima between two lattices
of Gaussians) and the project's 1e-4 m / 1e-4 rad against the restatement from the same start,
which the restatement's own float32 and float64 runs support (3.4e-7 apart from these hits: tests/test_d2d_search_ref.py).
"""
import ctypes as C
import math

import numpy as np
import pytest

import d2d_ref as R
import d2d_search_ref as S
from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import search, synth
from oracle import ndt2d as O

pytestmark = pytest.mark.gpu

DEG = math.pi / 180.0
OFFSET = (1.1, -0.9, 0.35)               # the guess of the loop closure: the generating pose plus this
BOX = (-27.0, -27.0, 27.0, 27.0)


CHUNK = 1024                             # components the score kernel stages per round (ALGORITHM.md section 2.15)


def _dist(p, q):
    return math.hypot(p[0] - q[0], p[1] - q[1]), abs(float(search.wrap(p[2] - q[2])))


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _same(a, b):
    return (a.pose == b.pose and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g) and a.score == b.score and
            a.iterations == b.iterations and a.n_hit == b.n_hit and a.status == b.status)


def _handles(d, **kw):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    t, s = NdtMatcher2D(**kw), NdtMatcher2D(**kw)
    t.set_target(d["tx"], d["ty"])
    s.set_target(d["sx"], d["sy"])
    return t, s


@pytest.fixture(scope="module")
def pair1():
    return synth.make_pair(1)


@pytest.fixture(scope="module")
def room50():
    return synth.make_pair(2, n_tgt=20_000, n_src=20_000)


def _loop_window(d):
    guess = tuple(a + b for a, b in zip(d["pose"], OFFSET))
    return guess, search.Window(guess, (2.0, 2.0, math.pi), (0.25, 0.25, 4.0 * DEG))


# ---------------------------------------------------------------------------------------------- 1. the volume
VOLUME_CASES = {
    # name: (pair, cell_size, window of the pair)
    "room8": ("pair1", 0.5, lambda d: search.Window(d["init"], (1.0, 1.0, math.pi), (0.1, 0.1, 10.0 * DEG))),
    # 1065 components: more than one staging chunk, and not a multiple of the inner unroll of four
    "room50": ("room50", 0.5, lambda d: search.Window(d["init"], (1.0, 1.0, math.pi), (0.25, 0.25, 20.0 * DEG))),
    # a finer grid on the 50 m room: several chunks
    "room50_fine": ("room50", 0.25, lambda d: search.Window(d["init"], (0.5, 0.5, 0.4), (0.125, 0.125, 0.1))),
    # a few hundred components short of a chunk, count odd
    "room50_coarse": ("room50", 1.0, lambda d: search.Window(d["init"], (1.0, 1.0, math.pi), (0.5, 0.5, 30.0 * DEG))),
}


@pytest.mark.parametrize("case", sorted(VOLUME_CASES))
def test_volume_matches_the_restatement(gpu_lib, request, case):
    pair, cell, win = VOLUME_CASES[case]
    d = request.getfixturevalue(pair)
    window = win(d)
    prm = O.NdtParams(cell_size=cell)
    tgt, _ = R.build_map(d["tx"], d["ty"], prm)
    _, comps = R.build_map(d["sx"], d["sy"], prm)
    if case == "room8":
        assert search.dims(window)[0] == (36, 21, 21)
    if case == "room50_fine":
        assert comps.n > 2 * CHUNK
    if case == "room50":
        assert comps.n > CHUNK and comps.n % 4 != 0
    if case == "room50_coarse":
        assert comps.n < CHUNK and comps.n % 4 != 0
    ref = S.volume(tgt, comps, window, prm)
    t, s = _handles(d, cell_size=cell)
    try:
        assert s.components()[0].size == comps.n
        vol = t.search_map_scores(s, *window).cpu().numpy().astype(np.float64)
    finally:
        t.close(); s.close()
    assert vol.shape == ref.shape
    err = np.abs(vol - ref)
    excess = float(np.max(err - 1e-4 * np.abs(ref)))
    print(f"{case}: {comps.n} components, lattice {vol.shape}, max(ref) {ref.max():.2f}, largest |vol - ref| {err.max():.3e} "
          f"(relative to max(ref) {err.max() / ref.max():.2e}), largest |vol - ref| - 1e-4 |ref| {excess:.3e}")
    assert np.max(ref) > 10.0                 # the window holds a real peak, not an empty map
    assert np.all(err <= 1e-4 * np.abs(ref) + 1e-3), excess


# ---------------------------------------------------------------------------------------------- 2. the hits
@pytest.mark.parametrize("case", ["cyclic", "window", "ties", "sparse"])
def test_hits_are_exactly_the_specification(gpu_lib, pair1, case):
    d = pair1
    c = d["init"]
    window, k, sep = {
        "cyclic": (search.Window(c, (1.0, 1.0, math.pi), (0.1, 0.1, 10.0 * DEG)), 16, (0.5, 0.1)),
        "window": (search.Window((c[0] + 0.1, c[1], 0.2), (0.5, 0.4, 0.3), (0.05, 0.05, 0.05)), 12, (0.2, 0.05)),
        # most of this window lies off the 8 m room: wide regions of score exactly 0
        "ties": (search.Window((10.0, 0.0, 0.0), (3.0, 1.0, 0.2), (0.25, 0.25, 0.1)), 64, (0.0, 0.0)),
        "sparse": (search.Window(c, (1.0, 1.0, math.pi), (0.1, 0.1, 10.0 * DEG)), 8, (100.0, 10.0)),
    }[case]
    t, s = _handles(d)
    try:
        vol = t.search_map_scores(s, *window).cpu().numpy()
        got = t.search_map(s, *window, k=k, min_sep=sep)
    finally:
        t.close(); s.close()
    want = search.select_hits(vol, window, k, sep)
    assert got == want
    assert got
    if case == "ties":
        assert np.count_nonzero(vol == 0) > vol.size // 4
    if case == "sparse":
        assert len(got) == 1 < k


# ---------------------------------------------------------------------------------------------- 3. the hit score
@pytest.mark.parametrize("pair", ["pair1", "room50"])
def test_hit_scores_are_evaluate_map_scores(gpu_lib, request, pair):
    d = request.getfixturevalue(pair)
    window = search.Window(d["init"], (1.0, 1.0, math.pi), (0.25, 0.25, 10.0 * DEG))
    t, s = _handles(d)
    try:
        hits = t.search_map(s, *window, k=8)
        assert len(hits) == 8
        for h in hits:
            ev = t.evaluate_map(s, h.pose)[2]
            print(f"{pair}: hit {h.index} score {h.score!r}, evaluate_map {ev!r}, relative difference {abs(h.score - ev) / abs(ev):.2e}")
            assert abs(h.score - ev) <= 1e-5 * abs(ev), (h, ev)
    finally:
        t.close(); s.close()


# ---------------------------------------------------------------------------------------------- 4. the purpose
def test_search_closes_a_loop_local_alignment_cannot(gpu_lib, room50):
    d = room50
    true = d["pose"]
    guess, window = _loop_window(d)
    prm = O.NdtParams()
    tgt, _ = R.build_map(d["tx"], d["ty"], prm)
    _, comps = R.build_map(d["sx"], d["sy"], prm)
    t, s = _handles(d)
    try:
        local = t.align_map(s, guess)
        out = t.search_align_map(s, *window, k=4)
    finally:
        t.close(); s.close()
    dt, dr = _dist(local.pose, true)
    print(f"align_map from the guess: status {local.status}, {dt:.3f} m / {dr:.3f} rad from the generating pose")
    assert dt > 1.0
    assert len(out) == 4
    conv = [(h, r) for h, r in out if r.converged]
    assert conv
    hit, best = max(conv, key=lambda hr: hr[1].score)
    dt, dr = _dist(best.pose, true)
    print(f"best: hit {hit.pose} score {hit.score:.2f} -> {best.pose} in {best.iterations} iterations, {dt:.4f} m / {dr:.2e} rad off")
    assert dt < 0.05 and dr < 0.005
    ref = R.align(tgt, comps, hit.pose, prm)
    err = np.abs(np.array(best.pose) - np.array(ref["pose"]))
    err[2] = abs(float(search.wrap(best.pose[2] - ref["pose"][2])))
    print(f"|pose - restatement from the same hit| {err}")
    assert ref["status"] == O.NDT_OK and err.max() < 1e-4


# ---------------------------------------------------------------------------------------------- 5. composition
def test_composition_and_determinism(gpu_lib, room50):
    d = room50
    _, window = _loop_window(d)
    t, s = _handles(d)
    try:
        out = t.search_align_map(s, *window, k=6)
        assert len(out) == 6
        for h, r in out:
            assert _same(r, t.align_map(s, h.pose)), (h, r)
        v1 = t.search_map_scores(s, *window)
        v2 = t.search_map_scores(s, *window)
        assert np.array_equal(_bits(v1), _bits(v2))
        h8 = t.search_map(s, *window, k=8)
        assert len(h8) == 8
        assert h8 == t.search_map(s, *window, k=8)
        assert h8[:6] == t.search_map(s, *window, k=6) == [h for h, _ in out]
    finally:
        t.close(); s.close()


# ---------------------------------------------------------------------------------------------- 6. the caches
@pytest.mark.parametrize("grow", ["source", "target"])
def test_the_volume_follows_the_grid(gpu_lib, room50, grow):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = room50
    window = search.Window(d["init"], (1.0, 1.0, 0.5), (0.25, 0.25, 0.1))
    half = d["tx"].size // 2
    clouds = {"target": (d["tx"], d["ty"]), "source": (d["sx"], d["sy"])}
    with NdtMatcher2D() as t, NdtMatcher2D() as s, NdtMatcher2D() as t2, NdtMatcher2D() as s2:
        hs = {"target": t, "source": s}
        for name, h in hs.items():
            x, y = clouds[name]
            h.reserve_target(*BOX)
            if name == grow:
                h.add_target_points(x[:half], y[:half])
            else:
                h.add_target_points(x, y)
        first = _bits(t.search_map_scores(s, *window))
        x, y = clouds[grow]
        hs[grow].add_target_points(x[half:], y[half:])
        second = _bits(t.search_map_scores(s, *window))
        for name, h in (("target", t2), ("source", s2)):
            h.reserve_target(*BOX)
            h.add_target_points(*clouds[name])
        fresh = _bits(t2.search_map_scores(s2, *window))
        assert np.array_equal(second, fresh)
        assert not np.array_equal(first, second)
        assert t.search_map(s, *window, k=8) == t2.search_map(s2, *window, k=8)
        # a new target through set_target drops the derived data as well
        t.set_target(d["sx"], d["sy"])
        t2.set_target(d["sx"], d["sy"])
        assert np.array_equal(_bits(t.search_map_scores(s, *window)), _bits(t2.search_map_scores(s2, *window)))


def test_a_saved_and_reloaded_pair_gives_the_live_bits(gpu_lib, room50):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = room50
    window = search.Window(d["init"], (1.0, 1.0, 0.5), (0.25, 0.25, 0.1))
    t, s = _handles(d)
    try:
        live = _bits(t.search_map_scores(s, *window))
        with NdtMatcher2D() as t2, NdtMatcher2D() as s2:
            # a handle that searched before it was loaded into: the load drops what it had derived
            t2.set_target(d["sx"], d["sy"])
            t2.search_map(t2, *window, k=2)
            t2.load_map(t.save_map())
            s2.load_map(s.save_map())
            assert np.array_equal(live, _bits(t2.search_map_scores(s2, *window)))
            assert t.search_map(s, *window, k=8) == t2.search_map(s2, *window, k=8)
    finally:
        t.close(); s.close()


# ---------------------------------------------------------------------------------------------- 7. no points
def test_maps_that_never_saw_a_point_search_and_align(gpu_lib, room50):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = room50
    true = d["pose"]
    _, window = _loop_window(d)
    t, s = _handles(d)
    try:
        maps = t.save_map(), s.save_map()
        live = t.search_align_map(s, *window, k=4)
    finally:
        t.close(); s.close()
    with NdtMatcher2D() as t2, NdtMatcher2D() as s2:
        t2.load_map(maps[0])
        s2.load_map(maps[1])
        out = t2.search_align_map(s2, *window, k=4)
    assert len(out) == len(live) == 4
    for (h, r), (h0, r0) in zip(out, live):
        assert h == h0 and _same(r, r0)
    hit, best = max(((h, r) for h, r in out if r.converged), key=lambda hr: hr[1].score)
    dt, dr = _dist(best.pose, true)
    assert dt < 0.05 and dr < 0.005


# ---------------------------------------------------------------------------------------------- 8. the error table
def _window(center, half, step, sep=(0.5, 0.1)):
    w = L.SearchWindow2D()
    for a in range(3):
        w.center[a], w.half_extent[a], w.step[a] = center[a], half[a], step[a]
    w.min_sep_trans, w.min_sep_rot = sep
    return w


def test_error_table_leaves_the_handles_intact(gpu_lib, pair1):
    import torch
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    lib = gpu_lib
    d = pair1
    sx, sy = torch.from_numpy(d["sx"]).cuda(), torch.from_numpy(d["sy"]).cuda()
    pwin = search.Window(d["init"], (0.5, 0.5, 0.2), (0.1, 0.1, 0.1))
    good = _window(d["init"], (0.5, 0.5, 0.2), (0.1, 0.1, 0.1))
    hits = (L.SearchHit2D * 64)()
    res = (L.Result2D * 64)()
    nh = C.c_int32(-1)
    vol = torch.empty((5, 11, 11), dtype=torch.float32, device="cuda")
    hp, rp, vp = C.cast(hits, C.c_void_p), C.cast(res, C.c_void_p), C.c_void_p(vol.data_ptr())

    def run(a, b, w=good, k=8, h=hp, n=nh):
        """the three entry points with the same arguments: they agree on the status"""
        ah, bh = (a._h if a is not None else None), (b._h if b is not None else None)
        wp = C.byref(w) if w is not None else None
        np_ = C.byref(n) if n is not None else None
        st = {lib.ndt2d_search_map(ah, bh, wp, k, h, np_), lib.ndt2d_search_align_map(ah, bh, wp, k, h, rp, np_)}
        if w is good and 1 <= k <= 64 and h is not None and n is not None:   # the volume call has no k, hits or count;
            st.add(lib.ndt2d_search_map_scores(ah, bh, wp, vp))              # `vol` holds the lattice of `good` only
        assert len(st) == 1, st
        return st.pop()

    with NdtMatcher2D() as t, NdtMatcher2D() as s, NdtMatcher2D() as empty, NdtMatcher2D(overlap_grids=4) as four, \
            NdtMatcher2D(min_points=100_000) as sparse:
        t.set_target(d["tx"], d["ty"])
        s.set_target(d["sx"], d["sy"])
        four.set_target(d["sx"], d["sy"])
        sparse.set_target(d["sx"], d["sy"])
        before = [(t.align_map(s, d["init"]), s.align_map(t, (0.0, 0.0, 0.0)), t.search(sx, sy, *pwin, k=8),
                   s.search(sx, sy, *pwin, k=8), t.align(sx, sy, d["init"]))]

        def intact():
            now = (t.align_map(s, d["init"]), s.align_map(t, (0.0, 0.0, 0.0)), t.search(sx, sy, *pwin, k=8),
                   s.search(sx, sy, *pwin, k=8), t.align(sx, sy, d["init"]))
            b = before[0]
            assert _same(now[0], b[0]) and _same(now[1], b[1]) and now[2] == b[2] and now[3] == b[3] and _same(now[4], b[4])

        # null arguments
        for kw in (dict(a=None, b=s), dict(a=t, b=None), dict(a=t, b=s, w=None), dict(a=t, b=s, h=None), dict(a=t, b=s, n=None)):
            assert run(**kw) == L.NDT_ERR_INVALID_ARG
        assert lib.ndt2d_search_map_scores(t._h, s._h, C.byref(good), None) == L.NDT_ERR_INVALID_ARG
        assert lib.ndt2d_search_align_map(t._h, s._h, C.byref(good), 8, hp, None, C.byref(nh)) == L.NDT_ERR_INVALID_ARG
        intact()
        # k outside 1 .. 64
        for k in (0, 65, -1):
            assert run(t, s, k=k) == L.NDT_ERR_INVALID_ARG
        # the window errors of ndt2d_search
        bad = [_window(d["init"], (0.5, 0.5, 0.2), (0.0, 0.1, 0.1)),
               _window(d["init"], (-0.5, 0.5, 0.2), (0.1, 0.1, 0.1)),
               _window((math.nan, 0.0, 0.0), (0.5, 0.5, 0.2), (0.1, 0.1, 0.1)),
               _window(d["init"], (0.5, math.inf, 0.2), (0.1, 0.1, 0.1)),
               _window(d["init"], (0.5, 0.5, 0.2), (0.1, 0.1, -0.1)),
               _window(d["init"], (0.5, 0.5, 0.2), (0.1, 0.1, 0.1), (math.nan, 0.1))]
        for w in bad:
            assert run(t, s, w=w) == L.NDT_ERR_INVALID_ARG
        huge = _window((0.0, 0.0, 0.0), (50.0, 50.0, math.pi), (0.01, 0.01, 0.1))
        assert lib.ndt2d_search_map(t._h, s._h, C.byref(huge), 8, hp, C.byref(nh)) == L.NDT_ERR_CAPACITY
        intact()
        # no grid on either side
        for a, b in ((t, empty), (empty, s), (empty, empty)):
            assert run(a, b) == L.NDT_ERR_NO_TARGET
        intact()
        # overlapping grids on either side: refused with align_map's message
        for a, b in ((t, four), (four, s)):
            assert run(a, b) == L.NDT_ERR_INVALID_ARG
            assert b"map-to-map alignment does not take overlapping grids" in lib.ndt_last_error()
        intact()
        # handles on different devices (where there is a second device)
        if lib.ndt_device_count() >= 2:
            with NdtMatcher2D(device=1) as other:
                other.set_target(d["sx"], d["sy"])
                for a, b in ((t, other), (other, s)):
                    assert lib.ndt2d_search_map(a._h, b._h, C.byref(good), 8, hp, C.byref(nh)) == L.NDT_ERR_INVALID_ARG
                    assert b"one device" in lib.ndt_last_error()
            torch.cuda.set_device(0)
            intact()
        else:
            print("one device: the different-devices case cannot be built here")
        # an empty component list or a target without a valid cell: no special case - an all-zero volume, no hits
        for a, b in ((t, sparse), (sparse, s)):
            nh.value = -1
            assert run(a, b) == L.NDT_OK and nh.value == 0
            torch.cuda.synchronize()
            assert not vol.cpu().numpy().any()
        # a window far from the map: the same
        nh.value = -1
        assert run(t, s, w=_window((500.0, 500.0, 0.0), (1.0, 1.0, math.pi), (0.1, 0.1, 0.1))) == L.NDT_OK and nh.value == 0
        intact()
        # target == source is legal
        nh.value = -1
        assert run(t, t) == L.NDT_OK and nh.value > 0
        # and a good call between the others changes nothing either
        assert run(t, s) == L.NDT_OK and nh.value > 0
        intact()


# ---------------------------------------------------------------------------------------------- 9. self-search
def test_a_map_searched_against_itself_peaks_at_the_centre(gpu_lib, pair1):
    """The restatement's maximum over this window is the centre pose and unique (151 against 63.1:
    tests/test_d2d_search_ref.py)."""
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = pair1
    window = search.Window((0.0, 0.0, 0.0), (0.5, 0.5, math.pi), (0.1, 0.1, 10.0 * DEG))
    (nt, ny, nx), _ = search.dims(window)
    with NdtMatcher2D() as t:
        t.set_target(d["tx"], d["ty"])
        hits = t.search_map(t, *window, k=4)
        n = t.grid_info().n_valid
        out = t.search_align_map(t, *window, k=1)
    assert hits[0].pose == (0.0, 0.0, 0.0) and hits[0].index == ((ny - 1) // 2) * nx + (nx - 1) // 2
    assert hits[0].score == pytest.approx(n, rel=1e-5)
    assert out[0][0] == hits[0] and out[0][1].pose == (0.0, 0.0, 0.0) and out[0][1].iterations == 1
