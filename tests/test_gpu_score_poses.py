"""The score of a scan at a list of poses (ndt2d_score_poses*, ndt2d_best_poses*): against the float64 restatement
(tests/score_poses_ref.py), bit for bit the volume of the exhaustive search on its lattice, independent of the list's
shape, exact zeros for non-finite poses, the hits against search.select_best, the composition with the multi-start
chain, and the errors."""
import ctypes as C
import math

import numpy as np
import pytest

import score_poses_ref as R
from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import search, synth

pytestmark = pytest.mark.gpu

DEG = math.pi / 180.0
NAN, INF = math.nan, math.inf


def _dev(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in arrays)


def _list(poses):
    import torch
    return torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)).cuda()


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return (a.pose == b.pose and a.iterations == b.iterations and a.status == b.status and a.n_hit == b.n_hit
            and a.score == b.score and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g))


@pytest.fixture(scope="module")
def pair1():
    return synth.make_pair(1)


@pytest.fixture(scope="module")
def matcher(gpu_lib, pair1):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    with NdtMatcher2D() as m:
        m.set_target(pair1["tx"], pair1["ty"])
        yield m


@pytest.fixture(scope="module")
def near(pair1):
    """257 poses within +-1 m / +-pi of the fixture's pose, and that pose itself (fixed seed)."""
    rng = np.random.default_rng(20241)
    c = np.asarray(pair1["init"], dtype=np.float64)
    p = c[None, :] + rng.uniform(-1.0, 1.0, (257, 3)) * np.array([1.0, 1.0, math.pi])
    return np.concatenate([p, c[None, :]])


@pytest.fixture(scope="module")
def thousand(pair1):
    rng = np.random.default_rng(20242)
    c = np.asarray(pair1["init"], dtype=np.float64)
    return c[None, :] + rng.uniform(-1.0, 1.0, (1000, 3)) * np.array([0.5, 0.5, 0.5])


@pytest.mark.parametrize("overlap", [1, 4])
def test_scores_match_the_oracle(gpu_lib, pair1, near, overlap):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    from oracle import ndt2d as o
    d = pair1
    prm = o.NdtParams(overlap=overlap)
    ref = R.scores2d(o.build_grids(d["tx"], d["ty"], prm), d["sx"], d["sy"], near, prm)
    sx, sy = _dev(d["sx"], d["sy"])
    with NdtMatcher2D(overlap_grids=overlap) as m:
        m.set_target(d["tx"], d["ty"])
        got = m.score_poses(sx, sy, _list(near)).cpu().numpy()
        assert got.dtype == np.float32 and got.shape == (258,)
        err = np.abs(got.astype(np.float64) - ref)
        print("largest error over the bound:", float(np.max(err - (1e-4 * np.abs(ref) + 1e-3))), "max ref", ref.max())
        assert np.all(err <= 1e-4 * np.abs(ref) + 1e-3)
        assert np.max(ref) > 10.0
        for i in np.argsort(-got, kind="stable")[:8]:
            ev = m.evaluate(sx, sy, tuple(near[i]))[2]
            assert abs(float(got[i]) - ev) <= 1e-5 * abs(ev), (i, got[i], ev)


def _lattice_list(window):
    xs, ys, th = search.lattice(window)
    T, Y, X = np.meshgrid(th, ys, xs, indexing="ij")
    return np.stack([X.ravel(), Y.ravel(), T.ravel()], axis=1)


@pytest.mark.parametrize("overlap", [1, 4])
def test_a_lattice_given_as_a_list_is_the_search_volume_bit_for_bit(gpu_lib, pair1, overlap):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = pair1
    window = search.Window(d["init"], (1.0, 1.0, math.pi), (0.1, 0.1, 10.0 * DEG))
    poses = _list(_lattice_list(window))
    assert poses.shape[0] == 36 * 21 * 21
    big = [np.concatenate([a, a, a]) for a in (d["sx"], d["sy"])]
    assert big[0].size == 3000
    spliced = [a.copy() for a in big]
    spliced[0][[0, 7, 1500, 2047, 2048, 2999]] = np.nan
    spliced[1][[3, 7, 2046, 2500]] = np.nan
    spliced[0][11] = np.inf
    with NdtMatcher2D(overlap_grids=overlap) as m:
        m.set_target(d["tx"], d["ty"])
        for n in (1, 3, 4, 5, 1000, 2047, 2048, 2049, 3000):
            s = _dev(big[0][:n], big[1][:n])
            vol = m.search_scores(*s, *window)
            got = m.score_poses(*s, poses)
            assert np.array_equal(_bits(got), _bits(vol).reshape(-1)), n
        assert float(vol.max()) > 10.0
        s = _dev(*spliced)
        vol = m.search_scores(*s, *window)
        assert np.array_equal(_bits(m.score_poses(*s, poses)), _bits(vol).reshape(-1))
        assert float(vol.max()) > 10.0


def test_a_score_does_not_depend_on_the_list(matcher, pair1, thousand):
    import torch
    m = matcher
    sx, sy = _dev(pair1["sx"], pair1["sy"])
    full = _bits(m.score_poses(sx, sy, _list(thousand)))
    assert np.array_equal(full, _bits(m.score_poses(sx, sy, _list(thousand))))         # two calls, the same bits
    assert np.count_nonzero(full) > 900
    for k in (1, 63, 64, 65, 255, 256, 257, 1000):
        poses = _list(thousand[:k])
        out = torch.full((k + 64,), -7.0, dtype=torch.float32, device="cuda")
        m.wait_stream()
        st = m._c.score_poses_dev(m._h, sx.data_ptr(), sy.data_ptr(), sx.numel(), poses.data_ptr(), k, out.data_ptr())
        assert st == L.NDT_OK
        out = out.cpu().numpy()
        assert np.array_equal(out[:k].view(np.uint32), full[:k]), k
        assert np.all(out[k:] == -7.0), k                                               # the guard is untouched
    # the tail of the list, so that an entry changes its workgroup and its lane
    assert np.array_equal(_bits(m.score_poses(sx, sy, _list(thousand[301:]))), full[301:])
    perm = np.random.default_rng(5).permutation(1000)
    assert np.array_equal(_bits(m.score_poses(sx, sy, _list(thousand[perm]))), full[perm])


def _poisoned(thousand):
    bad = thousand[:300].copy()
    where = {}
    slots = iter([0, 1, 62, 63, 64, 65, 130, 255, 256, 299])
    for coord in range(3):
        for v in (NAN, INF, -INF):
            i = next(slots)
            bad[i, coord] = v
            where[i] = (coord, v)
    bad[299] = (NAN, INF, -INF)
    where[299] = None
    return bad, sorted(where)


def test_non_finite_poses_score_exactly_zero(matcher, pair1, thousand):
    m = matcher
    sx, sy = _dev(pair1["sx"], pair1["sy"])
    clean = _bits(m.score_poses(sx, sy, _list(thousand[:300])))
    bad, idx = _poisoned(thousand)
    assert len(idx) == 10
    got = _bits(m.score_poses(sx, sy, _list(bad)))
    assert np.all(got[idx] == 0)                                   # +0.0f: all bits clear
    assert np.all(clean[idx] != 0)
    rest = np.setdiff1d(np.arange(300), idx)
    assert np.array_equal(got[rest], clean[rest])
    host = m.score_poses(pair1["sx"], pair1["sy"], bad)
    assert np.array_equal(_bits(host), got)
    hits = m.best_poses(sx, sy, _list(bad), k=64, min_sep=(0.0, 0.0))
    assert len(hits) == 64 and not set(h.index for h in hits) & set(idx)


def test_finite_poses_beyond_float32_score_exactly_zero(matcher, pair1, thousand):
    """A finite pose whose float32 form is not finite is no pose either: a translation beyond float32's range scores
    +0.0f, and a heading too large to wrap (its double has no digits below a turn) scores +0.0f or what the heading it
    wraps to scores - never NaN, which would poison a particle filter's normalisation.  Neighbours are unchanged."""
    m = matcher
    sx, sy = _dev(pair1["sx"], pair1["sy"])
    clean = _bits(m.score_poses(sx, sy, _list(thousand[:130])))
    bad = thousand[:130].copy()
    absurd = {0: (0, 1e300), 63: (1, -1e39), 64: (2, 1e300), 65: (2, -1.7e308), 129: (2, 1e19)}
    for i, (coord, v) in absurd.items():
        bad[i, coord] = v
    got = m.score_poses(sx, sy, _list(bad)).cpu().numpy()
    assert np.isfinite(got).all() and np.all(got >= 0.0)            # whatever an absurd heading wraps to: never NaN
    idx = sorted(absurd)
    assert np.all(_bits(got)[[0, 63]] == 0)                         # the translations beyond float32: +0.0f
    rest = np.setdiff1d(np.arange(130), idx)
    assert np.array_equal(_bits(got)[rest], clean[rest])


CASES = {
    # duplicates: every pose three times
    "duplicates": (lambda d, t: np.concatenate([t[:200], t[:200], t[:200]]), ((0.0, 0.0), (0.5, 0.1), (100.0, 10.0)), (1, 16, 64)),
    # ties: the lattice of a window that lies mostly off the 8 m room, so most scores are 0 and many equal
    "ties": (lambda d, t: _lattice_list(search.Window((10.0, 0.0, 0.0), (3.0, 1.0, 0.2), (0.25, 0.25, 0.1))),
             ((0.0, 0.0), (0.5, 0.1), (100.0, 10.0)), (1, 16, 64)),
    "near": (lambda d, t: t, ((0.0, 0.0), (0.5, 0.1), (100.0, 10.0)), (1, 16, 64)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_hits_are_exactly_the_specification(matcher, pair1, thousand, case):
    m = matcher
    make, seps, ks = CASES[case]
    poses = make(pair1, thousand)
    sx, sy = _dev(pair1["sx"], pair1["sy"])
    dl = _list(poses)
    scores = m.score_poses(sx, sy, dl).cpu().numpy()
    if case == "ties":
        assert np.count_nonzero(scores == 0) > scores.size // 4 and np.count_nonzero(scores > 0) > 0
    for sep in seps:
        for k in ks:
            got = m.best_poses(sx, sy, dl, k=k, min_sep=sep)
            want = search.select_best(scores, poses, k, sep)
            assert got == want, (case, sep, k)
            assert got == m.best_poses(sx, sy, dl, k=k, min_sep=sep)
    assert len(m.best_poses(sx, sy, dl, k=8, min_sep=(100.0, 10.0))) == 1
    for h in m.best_poses(sx, sy, dl, k=8):
        assert h.pose == tuple(poses[h.index]) and np.float32(h.score) == scores[h.index]


def test_hits_among_more_candidates_than_the_shortlist_holds(matcher, pair1):
    m = matcher
    rng = np.random.default_rng(20243)
    c = np.asarray(pair1["init"], dtype=np.float64)
    poses = c[None, :] + rng.uniform(-1.0, 1.0, (8192, 3)) * np.array([0.3, 0.3, 0.2])
    poses[5000:5100] = poses[100:200]                              # equal keys' scores: the index decides
    sx, sy = _dev(pair1["sx"], pair1["sy"])
    dl = _list(poses)
    scores = m.score_poses(sx, sy, dl).cpu().numpy()
    assert np.count_nonzero(scores > 0) > search.SHORTLIST
    for sep, k in (((0.0, 0.0), 64), ((0.05, 0.02), 64), ((0.5, 0.1), 8)):
        assert m.best_poses(sx, sy, dl, k=k, min_sep=sep) == search.select_best(scores, poses, k, sep)
    # numpy input goes through an upload and gives the same hits
    assert m.best_poses(pair1["sx"], pair1["sy"], poses, k=8) == search.select_best(scores, poses, 8, (0.5, 0.1))


def test_composition_with_the_multi_start_chain(matcher, pair1, thousand):
    m = matcher
    sx, sy = _dev(pair1["sx"], pair1["sy"])
    dl = _list(thousand)
    hits = m.best_poses(sx, sy, dl, k=6, min_sep=(0.2, 0.05))
    out = m.best_poses_align(sx, sy, dl, k=6, min_sep=(0.2, 0.05))
    assert len(hits) == 6 and [h for h, _ in out] == hits
    multi = m.align_multi_start(sx, sy, [h.pose for h in hits])
    for (_, r), q in zip(out, multi):
        assert _same(r, q), (r, q)
    assert any(r.converged for _, r in out)
    dev = m.score_poses(sx, sy, dl)
    host = m.score_poses(pair1["sx"], pair1["sy"], thousand)
    assert isinstance(host, np.ndarray) and host.dtype == np.float32
    assert np.array_equal(_bits(dev), _bits(host))
    # a list far off the map: no positive score, no hit, nothing refined
    far = thousand + np.array([500.0, 500.0, 0.0])
    assert not m.score_poses(sx, sy, _list(far)).cpu().numpy().any()
    assert m.best_poses(sx, sy, _list(far)) == [] and m.best_poses_align(sx, sy, _list(far)) == []


def test_errors_leave_the_handle_intact(gpu_lib, pair1, thousand):
    import torch
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = pair1
    lib = gpu_lib
    sx, sy = _dev(d["sx"], d["sy"])
    n = sx.numel()
    dl = _list(thousand[:100])
    out = torch.zeros(100, dtype=torch.float32, device="cuda")
    hits = (L.SearchHit2D * 64)()
    res = (L.Result2D * 64)()
    nh = C.c_int32(-1)
    ptr = lambda t: None if t is None else t.data_ptr()

    def score(m, x=sx, y=sy, nn=n, p=dl, mm=100, o=out):
        return lib.ndt2d_score_poses_dev(m._h, ptr(x), ptr(y), nn, ptr(p), mm, ptr(o))

    def best(m, x=sx, y=sy, nn=n, p=dl, mm=100, sep=(0.5, 0.1), k=8, hp=hits, np_=nh, align=False, rp=res):
        h = C.cast(hp, C.c_void_p) if hp is not None else None
        c = C.byref(np_) if np_ is not None else None
        if align:
            return lib.ndt2d_best_poses_align_dev(m._h, ptr(x), ptr(y), nn, ptr(p), mm, sep[0], sep[1], k, h,
                                                  C.cast(rp, C.c_void_p) if rp is not None else None, c)
        return lib.ndt2d_best_poses_dev(m._h, ptr(x), ptr(y), nn, ptr(p), mm, sep[0], sep[1], k, h, c)

    with NdtMatcher2D() as fresh:
        assert score(fresh) == L.NDT_ERR_NO_TARGET and best(fresh) == L.NDT_ERR_NO_TARGET
        hx = np.zeros(100, np.float32)
        assert lib.ndt2d_score_poses(fresh._h, d["sx"].ctypes.data, d["sy"].ctypes.data, n, thousand.ctypes.data, 100,
                                     hx.ctypes.data) == L.NDT_ERR_NO_TARGET
        fresh.set_target(d["tx"], d["ty"])
        ref1 = fresh.align(sx, sy, d["init"])
    with NdtMatcher2D() as m:
        m.set_target(d["tx"], d["ty"])
        m.wait_stream()
        for kw in (dict(x=None), dict(y=None), dict(p=None), dict(o=None), dict(nn=0), dict(nn=2 ** 31), dict(mm=0)):
            assert score(m, **kw) == L.NDT_ERR_INVALID_ARG, kw
        assert score(m, mm=2 ** 25 + 1) == L.NDT_ERR_CAPACITY
        for kw in (dict(x=None), dict(p=None), dict(hp=None), dict(np_=None), dict(nn=0), dict(mm=0), dict(k=0), dict(k=65),
                   dict(sep=(NAN, 0.1)), dict(sep=(0.5, INF)), dict(sep=(-0.5, 0.1)), dict(sep=(0.5, -0.1))):
            assert best(m, **kw) == L.NDT_ERR_INVALID_ARG, kw
            assert best(m, align=True, **kw) == L.NDT_ERR_INVALID_ARG, kw
        assert best(m, align=True, rp=None) == L.NDT_ERR_INVALID_ARG
        assert best(m, mm=2 ** 25 + 1) == L.NDT_ERR_CAPACITY
        assert not out.cpu().numpy().any()
        # after the errors the handle aligns as a fresh one does, bit for bit
        assert _same(m.align(sx, sy, d["init"]), ref1)
        # a call between two alignments, and one issued while an asynchronous alignment is in flight
        assert score(m) == L.NDT_OK and out.cpu().numpy().max() > 10.0
        alone = _bits(out)
        assert best(m) == L.NDT_OK and nh.value > 0
        assert _same(m.align(sx, sy, d["init"]), ref1)
        m.align_async(sx, sy, d["init"])
        during = _bits(m.score_poses(sx, sy, dl))
        assert _same(m.finish(), ref1)
        assert np.array_equal(during, alone)
        m.align_async(sx, sy, d["init"])
        assert best(m) == L.NDT_OK and nh.value > 0
        assert _same(m.finish(), ref1)
    with NdtMatcher2D() as empty:
        empty.reserve_target(-10.0, -10.0, 10.0, 10.0)
        out.fill_(3.0)
        torch.cuda.synchronize()
        assert score(empty) == L.NDT_OK and not out.cpu().numpy().any()
        assert best(empty) == L.NDT_OK and nh.value == 0
