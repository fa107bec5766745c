"""The map-to-map score of a 2D submap at a list of poses (ndt2d_score_map_poses*, ndt2d_best_map_poses*;
docs/ALGORITHM.md section 2.21): against the float64 restatement (tests/d2d_pose_list_ref.py), bit for bit the volume of
ndt2d_search_map_scores on its lattice, independent of the list's shape, exact zeros for non-finite poses, the hits
against search.select_best, the composition with ndt2d_align_map, the derived data following the grid, stored maps, and
the error table.

Bounds.  Scores: |score - ref| <= 1e-4 |ref| + 1e-3, the project's bound for a float32 private-sum score
(tests/test_gpu_search_map.py); tests/test_d2d_pose_list_ref.py holds the restatement's own float32 form within a
quarter of it on the very lists scored here.  Best poses against ndt2d_evaluate_map: 1e-5 relative (the same float32
terms in another summation order)."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import d2d_pose_list_ref as P
from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import search
from oracle import ndt2d as O

pytestmark = pytest.mark.gpu

DEG = math.pi / 180.0
NAN, INF = math.nan, math.inf
BOX = (-27.0, -27.0, 27.0, 27.0)


def _list(poses):
    import torch
    return torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)).cuda()


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


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
def pair(gpu_lib):
    """(target, source) of the 50 m room at 0.5 m: 1065 source components, two staging rounds."""
    t, s = _handles(P.pair2("room50"))
    yield t, s
    t.close(); s.close()


@pytest.fixture(scope="module")
def three_hundred():
    """300 poses round the generating pose, near enough that almost all score."""
    return P.near_list(P.pair2("room50")["pose"], (0.4, 0.4, 0.3), 30254, n=299)


def _both(t, s, poses):
    sc, nh = t.score_map_poses(s, _list(poses), with_hits=True)
    return _bits(sc), nh.cpu().numpy()


# ---------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("name", ["2d_room50", "2d_room50_coarse", "2d_room50_fine", "2d_room8"])
def test_scores_and_counts_match_the_restatement(gpu_lib, name):
    _, pair_name, cell, _, _ = P.NEAR_CASES[name]
    tgt, comps, prm, poses = P.near_case(name)
    ref, ref_hit = P.scores2d(tgt, comps, poses, prm)
    t, s = _handles(P.pair2(pair_name), cell_size=cell)
    try:
        assert s.components()[0].size == comps.n
        sc, nh = t.score_map_poses(s, _list(poses), with_hits=True)
        got, nh = sc.cpu().numpy(), nh.cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (129,) and nh.dtype == np.uint32 and nh.shape == (129,)
        err = np.abs(got.astype(np.float64) - ref)
        print(f"{name}: largest share of the bound {float(np.max(err / (1e-4 * np.abs(ref) + 1e-3))):.3f}, max ref {ref.max():.1f}")
        assert np.all(err <= 1e-4 * np.abs(ref) + 1e-3)
        assert np.max(ref) > 10.0
        assert np.array_equal(nh.astype(np.int64), ref_hit)
        for i in np.argsort(-got, kind="stable")[:8]:
            ev = t.evaluate_map(s, tuple(poses[i]))
            assert abs(float(got[i]) - ev[2]) <= 1e-5 * abs(ev[2]), (i, got[i], ev[2])
            assert int(nh[i]) == ev[3]
    finally:
        t.close(); s.close()


# ---------------------------------------------------------------------------------------------- 2. the lattice
LATTICE_CASES = {
    # the windows of test_gpu_search_map.py's volume cases: (pair, cell size, window, components)
    "room8": ("room8", 0.5, lambda d: search.Window(d["init"], (1.0, 1.0, math.pi), (0.1, 0.1, 10.0 * DEG)), 116),
    "room50": ("room50", 0.5, lambda d: search.Window(d["init"], (1.0, 1.0, math.pi), (0.25, 0.25, 20.0 * DEG)), 1065),
    "room50_fine": ("room50", 0.25, lambda d: search.Window(d["init"], (0.5, 0.5, 0.4), (0.125, 0.125, 0.1)), 2135),
}


@pytest.mark.parametrize("case", sorted(LATTICE_CASES))
def test_a_lattice_given_as_a_list_is_the_search_volume_bit_for_bit(gpu_lib, case):
    pair_name, cell, win, n_comp = LATTICE_CASES[case]
    d = P.pair2(pair_name)
    window = win(d)
    poses = P.lattice_list(window)
    assert poses.shape[0] % 256 != 0
    t, s = _handles(d, cell_size=cell)
    try:
        assert s.components()[0].size == n_comp
        vol = t.search_map_scores(s, *window)
        sc, nh = t.score_map_poses(s, _list(poses), with_hits=True)
    finally:
        t.close(); s.close()
    assert poses.shape[0] == vol.numel() and float(vol.max()) > 10.0 and nh.cpu().numpy().max() > 10
    assert np.array_equal(_bits(sc), _bits(vol).reshape(-1))


# ---------------------------------------------------------------------------------------------- 3. independence
def test_a_score_does_not_depend_on_the_list(pair, three_hundred):
    import torch
    t, s = pair
    poses = three_hundred
    full, cnt = _both(t, s, poses)
    again, cnt2 = _both(t, s, poses)
    assert np.array_equal(full, again) and np.array_equal(cnt, cnt2)              # two calls, the same bits
    assert np.count_nonzero(full) > 250 and cnt.max() > 100
    assert np.array_equal(_bits(t.score_map_poses(s, _list(poses))), full)        # d_n_hit = NULL: the same scores
    for k in (1, 255, 256, 257):
        dl = _list(poses[:k])
        out = torch.full((k + 64,), -7.0, dtype=torch.float32, device="cuda")
        hit = torch.full((k + 64,), -7, dtype=torch.int32, device="cuda")
        t.wait_stream()
        assert t._c.score_map_poses_dev(t._h, s._h, dl.data_ptr(), k, out.data_ptr(), hit.data_ptr()) == L.NDT_OK
        out, hit = out.cpu().numpy(), hit.cpu().numpy()
        assert np.array_equal(out[:k].view(np.uint32), full[:k]) and np.array_equal(hit[:k].view(np.uint32), cnt[:k]), k
        assert np.all(out[k:] == -7.0) and np.all(hit[k:] == -7), k               # the guards are untouched
    perm = np.random.default_rng(5).permutation(300)
    a, b = _both(t, s, poses[perm])
    assert np.array_equal(a, full[perm]) and np.array_equal(b, cnt[perm])
    a, b = _both(t, s, np.concatenate([poses, poses]))
    assert np.array_equal(a, np.concatenate([full, full])) and np.array_equal(b, np.concatenate([cnt, cnt]))
    for i in range(300):                                                          # each pose alone
        a, b = _both(t, s, poses[i:i + 1])
        assert a[0] == full[i] and b[0] == cnt[i], i
    host, host_hit = t.score_map_poses(s, poses, with_hits=True)                  # the host form: the same bits
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and host_hit.dtype == np.uint32
    assert np.array_equal(_bits(host), full) and np.array_equal(host_hit, cnt)
    assert np.array_equal(_bits(t.score_map_poses(s, poses)), full)


# ---------------------------------------------------------------------------------------------- 4. non-finite entries
def test_non_finite_poses_score_exactly_zero(pair, three_hundred):
    t, s = pair
    clean, clean_hit = _both(t, s, three_hundred)
    bad = three_hundred.copy()
    idx = [0, 1, 63, 64, 65, 255, 256, 257, 299]
    for i, (coord, v) in zip(idx, itertools.product(range(3), (NAN, INF, -INF))):
        bad[i, coord] = v
    absurd = {10: (0, 1e300), 11: (1, -1e300), 70: (2, 1e300)}
    for i, (coord, v) in absurd.items():
        bad[i, coord] = v
    # a translation beyond float32, and an angle whose wrap leaves no finite sine and cosine: exactly +0.0f as well
    zero = idx + sorted(absurd)
    got, hit = _both(t, s, bad)
    print("at the absurd entries:", {i: (got.view(np.float32)[i], hit[i]) for i in sorted(absurd)})
    assert np.all(got[zero] == 0) and np.all(hit[zero] == 0)       # +0.0f: all bits clear
    assert np.all(clean[zero] != 0)
    assert np.isfinite(got.view(np.float32)).all() and np.all(got.view(np.float32) >= 0.0)      # no entry gives a NaN
    rest = np.setdiff1d(np.arange(300), idx + sorted(absurd))
    assert np.array_equal(got[rest], clean[rest]) and np.array_equal(hit[rest], clean_hit[rest])
    hits = t.best_map_poses(s, _list(bad), k=64, min_sep=(0.0, 0.0))
    assert len(hits) == 64 and not set(h.index for h in hits) & set(zero)
    assert all(math.isfinite(h.score) and h.score > 0.0 for h in hits)


# ---------------------------------------------------------------------------------------------- 5. the hits
CASES = {
    "spread": (lambda t: t, ((0.5, 0.1), (0.0, 0.0), (0.2, 0.05)), (1, 8, 64)),
    "doubled": (lambda t: np.concatenate([t, t]), ((0.0, 0.0),), (1, 16, 64)),
    # from 52 m on the 50 m room's image has left the room's grid: wide regions of score exactly 0
    "off_the_map": (lambda t: P.lattice_list(search.Window((50.0, 0.0, 0.0), (12.0, 2.0, 0.2), (1.0, 1.0, 0.1))),
                    ((0.0, 0.0), (0.5, 0.1)), (8, 64)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_hits_are_exactly_the_specification(pair, three_hundred, case):
    t, s = pair
    make, seps, ks = CASES[case]
    poses = make(three_hundred)
    dl = _list(poses)
    scores = t.score_map_poses(s, dl).cpu().numpy()
    assert np.count_nonzero(scores > 0) > 0
    if case == "off_the_map":
        assert np.count_nonzero(scores == 0) > scores.size // 4
    for sep in seps:
        for k in ks:
            got = t.best_map_poses(s, dl, k=k, min_sep=sep)
            assert got == search.select_best(scores, poses, k, sep), (case, sep, k)
    if case == "doubled":                                           # exact ties go to the lower index
        got = t.best_map_poses(s, dl, k=16, min_sep=(0.0, 0.0))
        assert [h.index for h in got[1::2]] == [h.index + 300 for h in got[0::2]]
        assert [h.score for h in got[1::2]] == [h.score for h in got[0::2]]
    one = t.best_map_poses(s, dl, k=8, min_sep=(100.0, 10.0))
    assert len(one) == 1 and one == search.select_best(scores, poses, 8, (100.0, 10.0))
    for h in t.best_map_poses(s, dl, k=8):
        assert len(h.pose) == 3 and h.pose == tuple(poses[h.index]) and np.float32(h.score) == scores[h.index]


def test_a_list_without_a_positive_score_gives_no_hit(pair, three_hundred):
    t, s = pair
    far = three_hundred + np.array([500.0, 500.0, 0.0])
    sc, nh = _both(t, s, far)
    assert not sc.any() and not nh.any()
    assert t.best_map_poses(s, _list(far)) == [] and t.best_map_poses_align(s, _list(far)) == []


# ---------------------------------------------------------------------------------------------- 6. composition
def test_composition_with_align_map(pair, three_hundred):
    t, s = pair
    dl = _list(three_hundred)
    h8 = t.best_map_poses(s, dl, k=8, min_sep=(0.2, 0.05))
    out = t.best_map_poses_align(s, dl, k=6, min_sep=(0.2, 0.05))
    assert len(h8) == 8 and len(out) == 6
    assert [h for h, _ in out] == h8[:6] == t.best_map_poses(s, dl, k=6, min_sep=(0.2, 0.05))
    for h, r in out:
        assert _same(r, t.align_map(s, h.pose)), (h, r)
    # as a host list too
    assert t.best_map_poses(s, three_hundred, k=8, min_sep=(0.2, 0.05)) == h8


# ---------------------------------------------------------------------------------------------- 8. caches, stored maps
@pytest.mark.parametrize("grow", ["source", "target"])
def test_the_scores_follow_the_grid(gpu_lib, three_hundred, grow):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = P.pair2("room50")
    half = d["tx"].size // 2
    clouds = {"target": (d["tx"], d["ty"]), "source": (d["sx"], d["sy"])}
    with NdtMatcher2D() as t, NdtMatcher2D() as s, NdtMatcher2D() as t2, NdtMatcher2D() as s2:
        hs = {"target": t, "source": s}
        for name, h in hs.items():
            h.reserve_target(*BOX)
            if name == grow:
                h.add_target_points(*(a[:half] for a in clouds[name]))
            else:
                h.add_target_points(*clouds[name])
        first = _both(t, s, three_hundred)
        hs[grow].add_target_points(*(a[half:] for a in clouds[grow]))
        second = _both(t, s, three_hundred)
        for name, h in (("target", t2), ("source", s2)):
            h.reserve_target(*BOX)
            h.add_target_points(*clouds[name])
        fresh = _both(t2, s2, three_hundred)
        assert np.array_equal(second[0], fresh[0]) and np.array_equal(second[1], fresh[1])
        assert not np.array_equal(first[0], second[0])


def test_a_saved_and_reloaded_pair_gives_the_live_bits(pair, three_hundred):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    t, s = pair
    live = _both(t, s, three_hundred)
    with NdtMatcher2D() as t2, NdtMatcher2D() as s2:
        t2.load_map(t.save_map())
        s2.load_map(s.save_map())
        stored = _both(t2, s2, three_hundred)
        assert np.array_equal(live[0], stored[0]) and np.array_equal(live[1], stored[1])
        dl = _list(three_hundred)
        assert t.best_map_poses(s, dl, k=8) == t2.best_map_poses(s2, dl, k=8)


def test_a_map_against_itself_at_the_zero_pose(pair):
    t, _ = pair
    n = t.grid_info().n_valid
    sc, nh = t.score_map_poses(t, _list([(0.0, 0.0, 0.0), (500.0, 0.0, 0.0)]), with_hits=True)
    sc, nh = sc.cpu().numpy(), nh.cpu().numpy()
    assert n > 500 and int(nh[0]) == n and nh[1] == 0 and sc[1] == 0.0
    assert float(sc[0]) == pytest.approx(O.NdtParams().d1 * n, rel=1e-5)


# ---------------------------------------------------------------------------------------------- 9. the error table
def test_error_table_leaves_the_handles_intact(gpu_lib, three_hundred):
    import torch
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    lib = gpu_lib
    d = P.pair2("room50")
    pwin = search.Window(d["init"], (0.5, 0.5, 0.2), (0.25, 0.25, 0.1))
    dl = _list(three_hundred[:100])
    out = torch.zeros(100, dtype=torch.float32, device="cuda")
    cnt = torch.zeros(100, dtype=torch.int32, device="cuda")
    hits = (L.SearchHit2D * 64)()
    res = (L.Result2D * 64)()
    nh = C.c_int32(-1)
    ptr = lambda x: None if x is None else x.data_ptr()

    def score(a, b, p=dl, mm=100, o=out, n=cnt):
        return lib.ndt2d_score_map_poses_dev(a._h if a else None, b._h if b else None, ptr(p), mm, ptr(o), ptr(n))

    def best(a, b, p=dl, mm=100, sep=(0.5, 0.1), k=8, hp=hits, np_=nh, align=False, rp=res):
        h = C.cast(hp, C.c_void_p) if hp is not None else None
        cc = C.byref(np_) if np_ is not None else None
        ah, bh = (a._h if a else None), (b._h if b else None)
        if align:
            return lib.ndt2d_best_map_poses_align_dev(ah, bh, ptr(p), mm, sep[0], sep[1], k, h,
                                                      C.cast(rp, C.c_void_p) if rp is not None else None, cc)
        return lib.ndt2d_best_map_poses_dev(ah, bh, ptr(p), mm, sep[0], sep[1], k, h, cc)

    def every(a, b):
        """the entry points with the same handles: they agree on the status"""
        hx, hn = np.zeros(100, np.float32), np.zeros(100, np.uint32)
        st = {score(a, b), best(a, b), best(a, b, align=True),
              lib.ndt2d_score_map_poses(a._h, b._h, three_hundred.ctypes.data, 100, hx.ctypes.data, hn.ctypes.data)}
        assert len(st) == 1, st
        return st.pop()

    with NdtMatcher2D() as t, NdtMatcher2D() as s, NdtMatcher2D() as empty, NdtMatcher2D(overlap_grids=4) as four, \
            NdtMatcher2D(min_points=100_000) as sparse:
        t.set_target(d["tx"], d["ty"])
        s.set_target(d["sx"], d["sy"])
        four.set_target(d["sx"], d["sy"])
        sparse.set_target(d["sx"], d["sy"])
        assert sparse.grid_info().n_valid == 0

        def state():
            return (t.align_map(s, d["init"]), s.align_map(t, (0.0,) * 3), t.search_map(s, *pwin, k=8), s.search_map(t, *pwin, k=8))

        before = state()
        assert before[2]

        def intact():
            now = state()
            assert _same(now[0], before[0]) and _same(now[1], before[1]) and now[2] == before[2] and now[3] == before[3]

        t.wait_stream()
        # null arguments, m = 0
        for kw in (dict(a=None, b=s), dict(a=t, b=None), dict(a=t, b=s, p=None), dict(a=t, b=s, o=None), dict(a=t, b=s, mm=0)):
            assert score(**kw) == L.NDT_ERR_INVALID_ARG, kw
        assert score(t, s, mm=2 ** 25 + 1) == L.NDT_ERR_CAPACITY and b"2^25" in lib.ndt_last_error()
        # ... k outside 1..64, the separations; *n_hits is 0 wherever it could be written
        for kw in (dict(a=None, b=s), dict(a=t, b=None), dict(a=t, b=s, p=None), dict(a=t, b=s, hp=None), dict(a=t, b=s, mm=0),
                   dict(a=t, b=s, k=0), dict(a=t, b=s, k=65), dict(a=t, b=s, k=-1), dict(a=t, b=s, sep=(NAN, 0.1)),
                   dict(a=t, b=s, sep=(0.5, INF)), dict(a=t, b=s, sep=(-0.5, 0.1)), dict(a=t, b=s, sep=(0.5, -0.1))):
            for align in (False, True):
                nh.value = -1
                assert best(align=align, **kw) == L.NDT_ERR_INVALID_ARG, kw
                assert nh.value == 0, kw
        assert best(t, s, np_=None) == L.NDT_ERR_INVALID_ARG and best(t, s, np_=None, align=True) == L.NDT_ERR_INVALID_ARG
        nh.value = -1
        assert best(t, s, align=True, rp=None) == L.NDT_ERR_INVALID_ARG and nh.value == 0
        nh.value = -1
        assert best(t, s, mm=2 ** 25 + 1) == L.NDT_ERR_CAPACITY and nh.value == 0
        assert not out.cpu().numpy().any() and not cnt.cpu().numpy().any()
        intact()
        # no grid on either side; overlapping grids on either side
        for a, b in ((t, empty), (empty, s), (empty, empty)):
            assert every(a, b) == L.NDT_ERR_NO_TARGET
        for a, b in ((t, four), (four, s), (four, four)):
            assert every(a, b) == L.NDT_ERR_INVALID_ARG
            assert b"overlapping grids" in lib.ndt_last_error()
        intact()
        # handles on different devices (where there is a second device)
        if lib.ndt_device_count() >= 2:
            with NdtMatcher2D(device=1) as other:
                other.set_target(d["sx"], d["sy"])
                for a, b in ((t, other), (other, s)):
                    assert best(a, b) == L.NDT_ERR_INVALID_ARG
                    assert b"one device" in lib.ndt_last_error()
            torch.cuda.set_device(0)
            intact()
        else:
            print("one device: the different-devices case cannot be built here")
        # an empty component list or a target without a valid cell: no special case - zeros, no hits
        for a, b in ((t, sparse), (sparse, s)):
            nh.value = -1
            out.fill_(1.0)
            cnt.fill_(1)
            torch.cuda.synchronize()
            assert every(a, b) == L.NDT_OK and nh.value == 0
            assert not out.cpu().numpy().any() and not cnt.cpu().numpy().any()
        intact()
        # target == source is legal; a good call between the others, and one while an alignment is in flight
        nh.value = -1
        assert every(t, t) == L.NDT_OK and nh.value > 0
        assert every(t, s) == L.NDT_OK and nh.value > 0 and out.cpu().numpy().max() > 10.0
        alone = _bits(out)
        sx = [torch.from_numpy(np.ascontiguousarray(d[k], dtype=np.float32)).cuda() for k in ("sx", "sy")]
        ref = t.align(*sx, d["init"])
        t.align_async(*sx, d["init"])
        during = _bits(t.score_map_poses(s, dl))
        assert _same(t.finish(), ref) and np.array_equal(during, alone)
        intact()
