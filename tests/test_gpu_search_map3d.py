"""Exhaustive pose search for 3D map-to-map alignment on the device (ndt3d_search_map / ndt3d_search_map_scores /
ndt3d_search_align_map; docs/ALGORITHM.md section 2.16): the score volume against the float64 restatement
(tests/d2d3_search_ref.py), the hits against the numpy specification (gtsam_ndt_amd/search.py), the composition with
ndt3d_align_map, determinism, the derived data following the grid, maps that never saw a point, and the error table.

Bounds.  Volume: |vol - ref| <= 1e-4 |ref| + 1e-3, the project's bound for a float32 private-sum score volume
(tests/test_gpu_search.py).  Before relying on it the restatement's own float32 form (d2d3_ref.evaluate(...,
mirror32=True), every per-component operation rounded to float32) was held against its float64 form at every pose of
the five lattices of VOLUME_CASES, on the CPU: the largest |float32 - float64| is MIRROR32_WORST below, the largest
excess over 1e-4 |ref| is negative everywhere, so the float32 form stays within a quarter of the bound and the bound
is kept as it is.  Hit scores: 1e-5 relative against ndt3d_evaluate_map (the same float32 terms in another summation
order, ALGORITHM.md section 2.16).  Poses: 0.05 m / 0.005 rad of the generating pose (the centimetre-scale optima between
two lattices of Gaussians) and the project's 1e-4 m / 1e-4 rad against the restatement from the
same start, which the restatement's own float32 and float64 runs support (8.4e-6 apart from these hits:
tests/test_d2d3_search_ref.py).
"""
import ctypes as C
import math

import numpy as np
import pytest

import d2d3_ref as R
import d2d3_search_ref as S
from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import search, synth3d
from oracle import ndt3d as O

pytestmark = pytest.mark.gpu

DEG = math.pi / 180.0
POSE = (2.0, -1.5, 0.02, 0.004, -0.003, 0.6)         # the generating pose of the pairs
OFFSET = (1.6, -1.3, 0.0, 0.0, 0.0, 0.5)             # the guess of the loop closure: the generating pose plus this
CHUNK = 512                                          # components the score kernel stages per round (ALGORITHM.md section 2.16)
TILE = 16                                            # translations per workgroup and axis
# the restatement's float32 form against its float64 form over the lattices of VOLUME_CASES (see the module docstring):
# largest absolute difference, and that difference as a share of the bound 1e-4 |ref| + 1e-3 at its pose
MIRROR32_WORST = (4.7e-4, 0.061)
_cache = {}


def _pair(size):
    if size not in _cache:
        ne, na = {"small": (32, 1024), "full": (64, 2048)}[size]
        _cache[size] = synth3d.make_pair3d(n_elev=ne, n_azim=na, pose=POSE)
    return _cache[size]


def _ref_maps(size, cell):
    if (size, cell) not in _cache:
        d = _pair(size)
        prm = O.Ndt3Params(cell_size=cell)
        tgt, tcomps = R.build_map(d["tx"], d["ty"], d["tz"], prm)
        _, comps = R.build_map(d["sx"], d["sy"], d["sz"], prm)
        _cache[(size, cell)] = (tgt, tcomps, comps, prm)
    return _cache[(size, cell)]


def _dist(p, q):
    dt = math.sqrt(sum((p[a] - q[a]) ** 2 for a in range(3)))
    return dt, max(abs(float(search.wrap(p[a] - q[a]))) for a in range(3, 6))


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _same(a, b):
    return (a.pose == b.pose and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g) and a.score == b.score and
            a.iterations == b.iterations and a.n_hit == b.n_hit and a.status == b.status)


def _handles(size="small", cell=1.0, **kw):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = _pair(size)
    t, s = NdtMatcher3D(cell_size=cell, **kw), NdtMatcher3D(cell_size=cell, **kw)
    t.set_target(d["tx"], d["ty"], d["tz"])
    s.set_target(d["sx"], d["sy"], d["sz"])
    return t, s


def _loop_window():
    guess = tuple(a + b for a, b in zip(POSE, OFFSET))
    return guess, search.Window(guess, (3.0, 3.0, math.pi), (0.5, 0.5, 4.0 * DEG))


def _near(dx=0.0, dy=0.0, z=POSE[2], roll=POSE[3], pitch=POSE[4], dyaw=0.0):
    return (POSE[0] + dx, POSE[1] + dy, z, roll, pitch, POSE[5] + dyaw)


# ---------------------------------------------------------------------------------------------- 1. the volume
VOLUME_CASES = {
    # name: (pair, cell size, window, lattice, components)
    # more components than one staging chunk, count not a multiple of four; a lattice of 2 x 2 tiles, neither side a
    # multiple of the tile; a cyclic yaw axis
    "m1_cyclic": ("small", 1.0, search.Window(_near(0.2, -0.1), (2.5, 2.25, math.pi), (0.25, 0.25, 45.0 * DEG)), (8, 19, 21), 1198),
    # 1235 = 3 mod 4; a lattice smaller than one tile; a windowed yaw axis; non-zero roll and pitch and a z offset, so
    # the full R and the staged z / layer key are in play
    "half_tilted": ("small", 0.5, search.Window(_near(0.1, 0.1, 0.1, 0.05, -0.04, 0.02), (0.75, 0.75, 0.1), (0.125, 0.125, 0.05)),
                    (5, 13, 13), 1235),
    # fewer components than a chunk, count odd
    "m2_short": ("small", 2.0, search.Window(_near(-0.3, 0.2), (3.0, 3.0, math.pi), (0.5, 0.5, 30.0 * DEG)), (12, 13, 13), 509),
    # at least three chunks (four: 1907 components), tilted, windowed, 2 x 2 tiles
    "full_1m": ("full", 1.0, search.Window(_near(0.1, -0.2, 0.08, 0.05, -0.04, -0.03), (2.5, 2.25, 0.1), (0.25, 0.25, 0.1)),
                (3, 19, 21), 1907),
    # the centre several voxels above the map: every image fails the inside test in z at staging
    "above": ("small", 1.0, search.Window(_near(0.0, 0.0, 14.0, 0.05, -0.04), (1.5, 1.5, math.pi), (0.25, 0.25, 90.0 * DEG)),
              (4, 13, 13), 1198),
}


@pytest.mark.parametrize("case", sorted(VOLUME_CASES))
def test_volume_matches_the_restatement(gpu_lib, case):
    size, cell, window, lattice, n_comp = VOLUME_CASES[case]
    tgt, _, comps, prm = _ref_maps(size, cell)
    (nt, ny, nx), cyclic = search.dims(window)
    assert (nt, ny, nx) == lattice and comps.n == n_comp
    if case == "m1_cyclic":
        assert comps.n > CHUNK and comps.n % 4 != 0 and cyclic
        assert nx > TILE and ny > TILE and nx % TILE != 0 and ny % TILE != 0
    if case == "half_tilted":
        assert comps.n > CHUNK and comps.n % 4 == 3 and not cyclic
        assert nx < TILE and ny < TILE
        assert window.center[3] != 0.0 and window.center[4] != 0.0 and window.center[2] != POSE[2]
    if case == "m2_short":
        assert comps.n < CHUNK and comps.n % 2 == 1
    if case == "full_1m":
        assert comps.n > 2 * CHUNK and not cyclic and window.center[3] != 0.0 and window.center[4] != 0.0
    if case == "above":
        assert window.center[2] - (tgt.o[2] + tgt.dims[2] / tgt.inv_c) > 3.0 / tgt.inv_c      # voxels above the grid's top
    ref = S.volume(tgt, comps, window, prm)
    t, s = _handles(size, cell)
    try:
        assert s.components()[0].size == comps.n
        vol = t.search_map_scores(s, *window).cpu().numpy().astype(np.float64)
    finally:
        t.close(); s.close()
    assert vol.shape == ref.shape
    if case == "above":
        assert not ref.any() and not vol.any()
        return
    err = np.abs(vol - ref)
    excess = float(np.max(err - 1e-4 * np.abs(ref)))
    print(f"{case}: {comps.n} components, lattice {vol.shape}, max(ref) {ref.max():.2f}, largest |vol - ref| {err.max():.3e} "
          f"(relative to max(ref) {err.max() / ref.max():.2e}), largest |vol - ref| - 1e-4 |ref| {excess:.3e}")
    assert np.max(ref) > 10.0                 # the window holds a real peak, not an empty map
    assert np.all(err <= 1e-4 * np.abs(ref) + 1e-3), excess


def test_volume_matches_the_restatement_at_a_steep_pinned_roll_and_pitch(gpu_lib):
    """Roll 0.7 and pitch -0.5 pinned (VOLUME_CASES stays below 0.05): the small pair with its source map built from the
    scan seen from a frame tilted that far (tilted_cases.map_search_pair), 405 poses round the pose that puts it back.
    The same restatement, the same bound; tests/test_tilted_ref.py holds the restatement's float32 form within a quarter
    of it on this lattice."""
    import tilted_cases as T
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d, window = T.map_search_pair(), T.map_search_window()
    prm = O.Ndt3Params()
    tgt, _ = R.build_map(d["tx"], d["ty"], d["tz"], prm)
    _, comps = R.build_map(d["sx"], d["sy"], d["sz"], prm)
    assert search.dims(window)[0] == T.MAP_SEARCH_LATTICE and window.center[3:5] == (0.7, -0.5)
    ref = S.volume(tgt, comps, window, prm)
    with NdtMatcher3D() as t, NdtMatcher3D() as s:
        t.set_target(d["tx"], d["ty"], d["tz"])
        s.set_target(d["sx"], d["sy"], d["sz"])
        assert s.components()[0].size == comps.n
        vol = t.search_map_scores(s, *window).cpu().numpy().astype(np.float64)
    assert vol.shape == ref.shape
    err = np.abs(vol - ref)
    excess = float(np.max(err - 1e-4 * np.abs(ref)))
    print(f"steep: {comps.n} components, lattice {vol.shape}, max(ref) {ref.max():.2f}, largest |vol - ref| {err.max():.3e}, "
          f"largest |vol - ref| - 1e-4 |ref| {excess:.3e}")
    assert np.max(ref) > 10.0
    assert np.all(err <= 1e-4 * np.abs(ref) + 1e-3), excess


# ---------------------------------------------------------------------------------------------- 2. the hits
@pytest.mark.parametrize("case", ["cyclic", "window", "ties", "sparse"])
def test_hits_are_exactly_the_specification(gpu_lib, case):
    c = _near(0.2, -0.1)
    window, k, sep = {
        "cyclic": (search.Window(c, (2.0, 2.0, math.pi), (0.25, 0.25, 10.0 * DEG)), 16, (0.5, 0.1)),
        "window": (search.Window(_near(0.1, 0.0, 0.05, 0.01, -0.01, 0.1), (1.0, 0.75, 0.3), (0.125, 0.125, 0.05)), 12, (0.3, 0.05)),
        # most of this window lies off the 40 m room's 44 m grid: wide regions of score exactly 0
        "ties": (search.Window((40.0, 0.0, 0.02, 0.0, 0.0, 0.0), (12.0, 2.0, 0.2), (1.0, 1.0, 0.1)), 64, (0.0, 0.0)),
        "sparse": (search.Window(c, (2.0, 2.0, math.pi), (0.25, 0.25, 10.0 * DEG)), 8, (100.0, 10.0)),
    }[case]
    t, s = _handles()
    try:
        vol = t.search_map_scores(s, *window).cpu().numpy()
        got = t.search_map(s, *window, k=k, min_sep=sep)
    finally:
        t.close(); s.close()
    want = search.select_hits(vol, window, k, sep)
    assert got == want
    assert got
    assert all(h.pose[2:5] == tuple(window.center[2:5]) for h in got)
    if case == "ties":
        assert np.count_nonzero(vol == 0) > vol.size // 4
    if case == "sparse":
        assert len(got) == 1 < k


# ---------------------------------------------------------------------------------------------- 3. the hit score
@pytest.mark.parametrize("cell", [1.0, 0.5])
def test_hit_scores_are_evaluate_map_scores(gpu_lib, cell):
    window = search.Window(_near(0.2, -0.1, 0.05, 0.01, -0.01), (2.0, 2.0, math.pi), (0.5, 0.5, 10.0 * DEG))
    t, s = _handles("small", cell)
    try:
        hits = t.search_map(s, *window, k=8)
        assert len(hits) == 8
        for h in hits:
            ev = t.evaluate_map(s, h.pose)[2]
            print(f"{cell} m: hit {h.index} score {h.score!r}, evaluate_map {ev!r}, relative difference {abs(h.score - ev) / abs(ev):.2e}")
            assert abs(h.score - ev) <= 1e-5 * abs(ev), (h, ev)
    finally:
        t.close(); s.close()


# ---------------------------------------------------------------------------------------------- 4. the purpose
def test_search_closes_a_loop_local_alignment_cannot(gpu_lib):
    true = _pair("small")["pose"]
    guess, window = _loop_window()
    tgt, _, comps, prm = _ref_maps("small", 1.0)
    assert search.dims(window)[0] == (90, 13, 13)
    t, s = _handles()
    try:
        local = t.align_map(s, guess)
        out = t.search_align_map(s, *window, k=4)
    finally:
        t.close(); s.close()
    dt, dr = _dist(local.pose, true)
    print(f"align_map from the guess: status {local.status}, {dt:.3f} m / {dr:.3f} rad from the generating pose")
    assert dt > 1.0
    assert len(out) == 4
    conv = [(h, r) for h, r in out if r.status == L.NDT_OK]
    assert conv
    hit, best = max(conv, key=lambda hr: hr[1].score)
    dt, dr = _dist(best.pose, true)
    print(f"best: hit {hit.pose} score {hit.score:.2f} -> {best.pose} in {best.iterations} iterations, {dt:.4f} m / {dr:.2e} rad off")
    assert dt < 0.05 and dr < 0.005
    ref = R.align(tgt, comps, hit.pose, prm)
    err = np.abs(np.array(best.pose) - np.array(ref["pose"]))
    err[3:] = np.abs(search.wrap(np.array(best.pose[3:]) - np.array(ref["pose"][3:])))
    print(f"|pose - restatement from the same hit| {err}")
    assert ref["status"] == O.NDT_OK and err.max() < 1e-4


# ---------------------------------------------------------------------------------------------- 5. composition
def test_composition_and_determinism(gpu_lib):
    _, window = _loop_window()
    t, s = _handles()
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
BOX = ((-32.0, -32.0, -3.0), (32.0, 32.0, 7.0))       # holds every point of both clouds


@pytest.mark.parametrize("grow", ["source", "target"])
def test_the_volume_follows_the_grid(gpu_lib, grow):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = _pair("small")
    window = search.Window(_near(0.2, -0.1), (1.0, 1.0, 0.2), (0.25, 0.25, 0.1))
    half = d["tx"].size // 2
    clouds = {"target": (d["tx"], d["ty"], d["tz"]), "source": (d["sx"], d["sy"], d["sz"])}
    with NdtMatcher3D() as t, NdtMatcher3D() as s, NdtMatcher3D() as t2, NdtMatcher3D() as s2:
        hs = {"target": t, "source": s}
        for name, h in hs.items():
            h.reserve_target(*BOX)
            if name == grow:
                h.add_target_points(*(a[:half] for a in clouds[name]))
            else:
                h.add_target_points(*clouds[name])
        first = _bits(t.search_map_scores(s, *window))
        hs[grow].add_target_points(*(a[half:] for a in clouds[grow]))
        second = _bits(t.search_map_scores(s, *window))
        for name, h in (("target", t2), ("source", s2)):
            h.reserve_target(*BOX)
            h.add_target_points(*clouds[name])
        fresh = _bits(t2.search_map_scores(s2, *window))
        assert np.array_equal(second, fresh)
        assert not np.array_equal(first, second)
        assert t.search_map(s, *window, k=8) == t2.search_map(s2, *window, k=8)
        # a new target through set_target drops the derived data as well
        t.set_target(*clouds["source"])
        t2.set_target(*clouds["source"])
        assert np.array_equal(_bits(t.search_map_scores(s, *window)), _bits(t2.search_map_scores(s2, *window)))


# ---------------------------------------------------------------------------------------------- 7. saved maps
def test_a_saved_and_reloaded_pair_gives_the_live_bits(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = _pair("small")
    window = search.Window(_near(0.2, -0.1), (1.0, 1.0, 0.2), (0.25, 0.25, 0.1))
    t, s = _handles()
    try:
        live = _bits(t.search_map_scores(s, *window))
        with NdtMatcher3D() as t2, NdtMatcher3D() as s2:
            # a handle that searched before it was loaded into: the load drops what it had derived
            t2.set_target(d["sx"], d["sy"], d["sz"])
            t2.search_map(t2, *window, k=2)
            t2.load_map(t.save_map())
            s2.load_map(s.save_map())
            assert np.array_equal(live, _bits(t2.search_map_scores(s2, *window)))
            assert t.search_map(s, *window, k=8) == t2.search_map(s2, *window, k=8)
    finally:
        t.close(); s.close()


def test_maps_that_never_saw_a_point_search_and_align(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    true = _pair("small")["pose"]
    _, window = _loop_window()
    t, s = _handles()
    try:
        maps = t.save_map(), s.save_map()
        live = t.search_align_map(s, *window, k=4)
    finally:
        t.close(); s.close()
    with NdtMatcher3D() as t2, NdtMatcher3D() as s2:
        t2.load_map(maps[0])
        s2.load_map(maps[1])
        out = t2.search_align_map(s2, *window, k=4)
    assert len(out) == len(live) == 4
    for (h, r), (h0, r0) in zip(out, live):
        assert h == h0 and _same(r, r0)
    hit, best = max(((h, r) for h, r in out if r.status == L.NDT_OK), key=lambda hr: hr[1].score)
    dt, dr = _dist(best.pose, true)
    assert dt < 0.05 and dr < 0.005


# ---------------------------------------------------------------------------------------------- 8. the error table
def _window(center, half, step, sep=(0.5, 0.1)):
    w = L.SearchWindow3D()
    for a in range(6):
        w.center[a] = center[a]
    for a in range(3):
        w.half_extent[a], w.step[a] = half[a], step[a]
    w.min_sep_trans, w.min_sep_rot = sep
    return w


def test_error_table_leaves_the_handles_intact(gpu_lib):
    import torch
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    lib = gpu_lib
    d = _pair("small")
    c = _near(0.2, -0.1)
    half, step = (0.5, 0.5, 0.2), (0.25, 0.25, 0.1)
    pwin = search.Window(c, half, step)
    good = _window(c, half, step)
    hits = (L.SearchHit3D * 64)()
    res = (L.Result3D * 64)()
    nh = C.c_int32(-1)
    vol = torch.empty((5, 5, 5), dtype=torch.float32, device="cuda")
    hp, rp, vp = C.cast(hits, C.c_void_p), C.cast(res, C.c_void_p), C.c_void_p(vol.data_ptr())

    def run(a, b, w=good, k=8, h=hp, n=nh):
        """the three entry points with the same arguments: they agree on the status"""
        ah, bh = (a._h if a is not None else None), (b._h if b is not None else None)
        wp = C.byref(w) if w is not None else None
        np_ = C.byref(n) if n is not None else None
        st = {lib.ndt3d_search_map(ah, bh, wp, k, h, np_), lib.ndt3d_search_align_map(ah, bh, wp, k, h, rp, np_)}
        if w is good and 1 <= k <= 64 and h is not None and n is not None:   # the volume call has no k, hits or count;
            st.add(lib.ndt3d_search_map_scores(ah, bh, wp, vp))              # `vol` holds the lattice of `good` only
        assert len(st) == 1, st
        return st.pop()

    with NdtMatcher3D() as t, NdtMatcher3D() as s, NdtMatcher3D() as empty, NdtMatcher3D(min_points=100_000) as sparse:
        t.set_target(d["tx"], d["ty"], d["tz"])
        s.set_target(d["sx"], d["sy"], d["sz"])
        sparse.set_target(d["sx"], d["sy"], d["sz"])
        assert sparse.grid_info().n_valid == 0

        def state():
            return (t.align_map(s, c), s.align_map(t, (0.0,) * 6), t.search_map(s, *pwin, k=8), s.search_map(t, *pwin, k=8))

        before = state()
        assert before[2]

        def intact():
            now = state()
            assert _same(now[0], before[0]) and _same(now[1], before[1]) and now[2] == before[2] and now[3] == before[3]

        # null arguments
        for kw in (dict(a=None, b=s), dict(a=t, b=None), dict(a=t, b=s, w=None), dict(a=t, b=s, h=None), dict(a=t, b=s, n=None)):
            assert run(**kw) == L.NDT_ERR_INVALID_ARG
        assert lib.ndt3d_search_map_scores(t._h, s._h, C.byref(good), None) == L.NDT_ERR_INVALID_ARG
        assert lib.ndt3d_search_align_map(t._h, s._h, C.byref(good), 8, hp, None, C.byref(nh)) == L.NDT_ERR_INVALID_ARG
        intact()
        # k outside 1 .. 64; *n_hits is 0 wherever the count could be written
        for k in (0, 65, -1):
            assert run(t, s, k=k) == L.NDT_ERR_INVALID_ARG
        # the window errors: a step <= 0, a negative extent
        bad = [_window(c, half, (0.0, 0.25, 0.1)), _window(c, half, (0.25, 0.25, -0.1)), _window(c, (-0.5, 0.5, 0.2), step)]
        # a non-finite value in each of the nine window numbers (x, y, yaw of centre, extent, step) ...
        for v in (math.nan, math.inf):
            for a in range(3):
                cc, hh, ss = list(c), list(half), list(step)
                cc[(0, 1, 5)[a]] = v
                hh[a] = v
                ss[a] = v
                bad += [_window(cc, half, step), _window(c, hh, step), _window(c, half, ss)]
            # ... and in each pinned coordinate
            for a in (2, 3, 4):
                cc = list(c)
                cc[a] = v
                bad.append(_window(cc, half, step))
        bad.append(_window(c, half, step, (math.nan, 0.1)))
        for w in bad:
            nh.value = -1
            assert run(t, s, w=w) == L.NDT_ERR_INVALID_ARG
            assert nh.value == 0
        huge = _window((0.0,) * 6, (50.0, 50.0, math.pi), (0.01, 0.01, 0.1))
        assert lib.ndt3d_search_map(t._h, s._h, C.byref(huge), 8, hp, C.byref(nh)) == L.NDT_ERR_CAPACITY
        intact()
        # no grid on either side
        for a, b in ((t, empty), (empty, s), (empty, empty)):
            assert run(a, b) == L.NDT_ERR_NO_TARGET
        intact()
        # handles on different devices (where there is a second device)
        if lib.ndt_device_count() >= 2:
            with NdtMatcher3D(device=1) as other:
                other.set_target(d["sx"], d["sy"], d["sz"])
                for a, b in ((t, other), (other, s)):
                    assert lib.ndt3d_search_map(a._h, b._h, C.byref(good), 8, hp, C.byref(nh)) == L.NDT_ERR_INVALID_ARG
                    assert b"one device" in lib.ndt_last_error()
            torch.cuda.set_device(0)
            intact()
        else:
            print("one device: the different-devices case cannot be built here")
        # an empty component list or a target without a valid voxel: no special case - an all-zero volume, no hits
        for a, b in ((t, sparse), (sparse, s)):
            nh.value = -1
            vol.fill_(1.0)
            torch.cuda.synchronize()
            assert run(a, b) == L.NDT_OK and nh.value == 0
            torch.cuda.synchronize()
            assert not vol.cpu().numpy().any()
        # a window far from the map: the same
        nh.value = -1
        assert run(t, s, w=_window((500.0, 500.0, 0.0, 0.0, 0.0, 0.0), (1.0, 1.0, math.pi), (0.25, 0.25, 0.1))) == L.NDT_OK
        assert nh.value == 0
        intact()
        # target == source is legal
        nh.value = -1
        assert run(t, t) == L.NDT_OK and nh.value > 0
        # and a good call between the others changes nothing either
        assert run(t, s) == L.NDT_OK and nh.value > 0
        intact()


# ---------------------------------------------------------------------------------------------- 9. self-search
def test_a_map_searched_against_itself_peaks_at_the_centre(gpu_lib):
    """The restatement's maximum over this window is the centre pose and unique (1705 against 893.7:
    tests/test_d2d3_search_ref.py)."""
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = _pair("small")
    zero = (0.0,) * 6
    window = search.Window(zero, (0.5, 0.5, math.pi), (0.5, 0.5, 10.0 * DEG))
    (nt, ny, nx), _ = search.dims(window)
    with NdtMatcher3D() as t:
        t.set_target(d["tx"], d["ty"], d["tz"])
        hits = t.search_map(t, *window, k=4)
        n = t.grid_info().n_valid
        d1 = t.evaluate_map(t, zero)[2] / n                  # the identity scores d1 per component (section 2.14)
        out = t.search_align_map(t, *window, k=1)
    assert n == 1705
    assert hits[0].pose == zero and hits[0].index == ((ny - 1) // 2) * nx + (nx - 1) // 2
    assert hits[0].score == pytest.approx(O.Ndt3Params().d1 * n, rel=1e-5)
    assert d1 == pytest.approx(O.Ndt3Params().d1, rel=1e-5)
    assert out[0][0] == hits[0] and out[0][1].pose == zero
