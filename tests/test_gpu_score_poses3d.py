"""The score of a scan at a list of 3D poses (ndt3d_score_poses*, ndt3d_best_poses*): against
oracle.ndt3d.evaluate3(mirror32=True) (tests/score_poses_ref.py), bit for bit the volume of the exhaustive search on its
lattice, independent of the list's shape, exact zeros for non-finite poses, the hits against search.select_best, the
composition with the multi-start chain, a search over z, roll and pitch that the lattice cannot do, and the errors."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest

import score_poses_ref as R
from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import search

pytestmark = pytest.mark.gpu

DEG = math.pi / 180.0
NAN, INF = math.nan, math.inf
GOLD3 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ndt3d_small.npz")


def _dev(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in arrays)


def _list(poses):
    import torch
    return torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 6)).cuda()


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    return (a.pose == b.pose and a.iterations == b.iterations and a.status == b.status and a.n_hit == b.n_hit
            and a.score == b.score and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g))


@pytest.fixture(scope="module")
def small():
    g = np.load(GOLD3)
    return {k: np.ascontiguousarray(g[k], dtype=np.float32) for k in ("tx", "ty", "tz", "sx", "sy", "sz")} | {
        "init": tuple(float(v) for v in g["init"]), "pose": tuple(float(v) for v in g["final_pose"])}


@pytest.fixture(scope="module")
def matcher(gpu_lib, small):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    with NdtMatcher3D() as m:
        m.set_target(small["tx"], small["ty"], small["tz"])
        yield m


@pytest.fixture(scope="module")
def scan(small):
    return _dev(small["sx"], small["sy"], small["sz"])


SPREAD = np.array([0.8, 0.8, 0.8, 0.1, 0.1, math.pi])


@pytest.fixture(scope="module")
def near(small):
    """257 poses within +-0.8 m / +-0.1 rad / any yaw of the fixture's pose, and that pose itself (fixed seed)."""
    rng = np.random.default_rng(30241)
    c = np.asarray(small["pose"], dtype=np.float64)
    return np.concatenate([c[None, :] + rng.uniform(-1.0, 1.0, (257, 6)) * SPREAD, c[None, :]])


@pytest.fixture(scope="module")
def thousand(small):
    rng = np.random.default_rng(30242)
    c = np.asarray(small["pose"], dtype=np.float64)
    return c[None, :] + rng.uniform(-1.0, 1.0, (1000, 6)) * np.array([0.4, 0.4, 0.2, 0.05, 0.05, 0.3])


def test_scores_match_the_oracle(matcher, small, scan, near):
    from oracle import ndt3d as o
    d = small
    m = matcher
    prm = o.Ndt3Params()
    ref = R.scores3d(o.build_grid3(d["tx"], d["ty"], d["tz"], prm), d["sx"], d["sy"], d["sz"], near, prm)
    got = m.score_poses(*scan, _list(near)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (258,)
    err = np.abs(got.astype(np.float64) - ref)
    print("largest error over the bound:", float(np.max(err - (1e-4 * np.abs(ref) + 1e-3))), "max ref", ref.max())
    assert np.all(err <= 1e-4 * np.abs(ref) + 1e-3)
    assert np.max(ref) > 10.0
    for i in np.argsort(-got, kind="stable")[:8]:
        ev = m.evaluate(*scan, tuple(near[i]))[2]
        assert abs(float(got[i]) - ev) <= 1e-5 * abs(ev), (i, got[i], ev)


def _lattice_list(window):
    c = window[0]
    xs, ys, th = search.lattice(window)
    T, Y, X = np.meshgrid(th, ys, xs, indexing="ij")
    one = np.ones(X.size)
    return np.stack([X.ravel(), Y.ravel(), c[2] * one, c[3] * one, c[4] * one, T.ravel()], axis=1)


def test_a_lattice_given_as_a_list_is_the_search_volume_bit_for_bit(matcher, small):
    d = small
    m = matcher
    c = (d["pose"][0] + 0.05, d["pose"][1] - 0.05, 0.04, 0.012, -0.008, d["pose"][5])
    window = search.Window(c, (0.8, 0.8, math.pi), (0.2, 0.2, 10.0 * DEG))
    poses = _list(_lattice_list(window))
    assert poses.shape[0] == 36 * 9 * 9
    cloud = [d["sx"], d["sy"], d["sz"]]
    assert cloud[0].size == 4096
    for n in (1, 3, 1023, 1024, 1025, 4096):
        s = _dev(*(a[:n] for a in cloud))
        vol = m.search_scores(*s, *window)
        assert np.array_equal(_bits(m.score_poses(*s, poses)), _bits(vol).reshape(-1)), n
    assert float(vol.max()) > 10.0
    spliced = [a.copy() for a in cloud]
    spliced[0][[0, 7, 1023, 1024, 4095]] = np.nan
    spliced[1][[3, 7, 2046]] = np.nan
    spliced[2][[5, 1025, 3000]] = np.nan
    spliced[2][11] = np.inf
    s = _dev(*spliced)
    vol = m.search_scores(*s, *window)
    assert np.array_equal(_bits(m.score_poses(*s, poses)), _bits(vol).reshape(-1))
    assert float(vol.max()) > 10.0


def test_a_score_does_not_depend_on_the_list(matcher, scan, thousand):
    import torch
    m = matcher
    full = _bits(m.score_poses(*scan, _list(thousand)))
    assert np.array_equal(full, _bits(m.score_poses(*scan, _list(thousand))))          # two calls, the same bits
    assert np.count_nonzero(full) > 900
    for k in (1, 63, 64, 65, 255, 256, 257, 1000):
        poses = _list(thousand[:k])
        out = torch.full((k + 64,), -7.0, dtype=torch.float32, device="cuda")
        m.wait_stream()
        st = m._c.score_poses_dev(m._h, *[a.data_ptr() for a in scan], scan[0].numel(), poses.data_ptr(), k, out.data_ptr())
        assert st == L.NDT_OK
        out = out.cpu().numpy()
        assert np.array_equal(out[:k].view(np.uint32), full[:k]), k
        assert np.all(out[k:] == -7.0), k                                               # the guard is untouched
    assert np.array_equal(_bits(m.score_poses(*scan, _list(thousand[301:]))), full[301:])
    perm = np.random.default_rng(5).permutation(1000)
    assert np.array_equal(_bits(m.score_poses(*scan, _list(thousand[perm]))), full[perm])


def test_non_finite_poses_score_exactly_zero(matcher, small, scan, thousand):
    m = matcher
    clean = _bits(m.score_poses(*scan, _list(thousand[:300])))
    bad = thousand[:300].copy()
    idx = [0, 1, 2, 62, 63, 64, 65, 66, 67, 128, 129, 130, 254, 255, 256, 257, 298, 299]
    for i, (coord, v) in zip(idx, itertools.product(range(6), (NAN, INF, -INF))):
        bad[i, coord] = v
    got = _bits(m.score_poses(*scan, _list(bad)))
    assert np.all(got[idx] == 0)                                   # +0.0f: all bits clear
    assert np.all(clean[idx] != 0)
    rest = np.setdiff1d(np.arange(300), idx)
    assert np.array_equal(got[rest], clean[rest])
    host = m.score_poses(small["sx"], small["sy"], small["sz"], bad)
    assert np.array_equal(_bits(host), got)
    hits = m.best_poses(*scan, _list(bad), k=64, min_sep=(0.0, 0.0))
    assert len(hits) == 64 and not set(h.index for h in hits) & set(idx)


def test_finite_poses_beyond_float32_score_exactly_zero(matcher, scan, thousand):
    """As in 2D: a translation beyond float32's range scores +0.0f; an angle too large to wrap scores +0.0f or what the
    angle it wraps to scores, never NaN.  Neighbours are unchanged."""
    m = matcher
    clean = _bits(m.score_poses(*scan, _list(thousand[:130])))
    bad = thousand[:130].copy()
    absurd = {0: (0, 1e300), 1: (2, 1e39), 63: (1, -1e39), 64: (3, 1e300), 65: (4, -1.7e308), 129: (5, 1e19)}
    for i, (coord, v) in absurd.items():
        bad[i, coord] = v
    got = m.score_poses(*scan, _list(bad)).cpu().numpy()
    assert np.isfinite(got).all() and np.all(got >= 0.0)
    assert np.all(_bits(got)[[0, 1, 63]] == 0)
    rest = np.setdiff1d(np.arange(130), sorted(absurd))
    assert np.array_equal(_bits(got)[rest], clean[rest])


CASES = {
    "duplicates": (lambda d, t: np.concatenate([t[:200], t[:200], t[:200]]), ((0.0, 0.0), (0.5, 0.1), (100.0, 10.0)), (1, 16, 64)),
    # ties: the lattice of a window that lies mostly off the 40 m room, so most scores are 0
    "ties": (lambda d, t: _lattice_list(search.Window((38.0, 0.0, 0.0, 0.0, 0.0, 0.0), (12.0, 4.0, 0.2), (1.0, 1.0, 0.1))),
             ((0.0, 0.0), (0.5, 0.1), (100.0, 10.0)), (1, 16, 64)),
    "near": (lambda d, t: t, ((0.0, 0.0), (0.5, 0.1), (100.0, 10.0)), (1, 16, 64)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_hits_are_exactly_the_specification(matcher, small, scan, thousand, case):
    m = matcher
    make, seps, ks = CASES[case]
    poses = make(small, thousand)
    dl = _list(poses)
    scores = m.score_poses(*scan, dl).cpu().numpy()
    if case == "ties":
        assert np.count_nonzero(scores == 0) > scores.size // 4 and np.count_nonzero(scores > 0) > 0
    for sep in seps:
        for k in ks:
            got = m.best_poses(*scan, dl, k=k, min_sep=sep)
            assert got == search.select_best(scores, poses, k, sep), (case, sep, k)
            assert got == m.best_poses(*scan, dl, k=k, min_sep=sep)
    assert len(m.best_poses(*scan, dl, k=8, min_sep=(100.0, 10.0))) == 1
    for h in m.best_poses(*scan, dl, k=8):
        assert len(h.pose) == 6 and h.pose == tuple(poses[h.index]) and np.float32(h.score) == scores[h.index]


def test_hits_among_more_candidates_than_the_shortlist_holds(matcher, small, scan):
    m = matcher
    rng = np.random.default_rng(30243)
    c = np.asarray(small["pose"], dtype=np.float64)
    poses = c[None, :] + rng.uniform(-1.0, 1.0, (8192, 6)) * np.array([0.3, 0.3, 0.15, 0.04, 0.04, 0.2])
    poses[5000:5100] = poses[100:200]                              # equal scores: the index decides
    dl = _list(poses)
    scores = m.score_poses(*scan, dl).cpu().numpy()
    assert np.count_nonzero(scores > 0) > search.SHORTLIST
    for sep, k in (((0.0, 0.0), 64), ((0.05, 0.02), 64), ((0.5, 0.1), 8)):
        assert m.best_poses(*scan, dl, k=k, min_sep=sep) == search.select_best(scores, poses, k, sep)
    assert m.best_poses(small["sx"], small["sy"], small["sz"], poses, k=8) == search.select_best(scores, poses, 8, (0.5, 0.1))


def test_composition_with_the_multi_start_chain(matcher, small, scan, thousand):
    m = matcher
    dl = _list(thousand)
    hits = m.best_poses(*scan, dl, k=6, min_sep=(0.2, 0.05))
    out = m.best_poses_align(*scan, dl, k=6, min_sep=(0.2, 0.05))
    assert len(hits) == 6 and [h for h, _ in out] == hits
    multi = m.align_multi_start(*scan, [h.pose for h in hits])
    for (_, r), q in zip(out, multi):
        assert _same(r, q), (r, q)
    dev = m.score_poses(*scan, dl)
    host = m.score_poses(small["sx"], small["sy"], small["sz"], thousand)
    assert isinstance(host, np.ndarray) and host.dtype == np.float32
    assert np.array_equal(_bits(dev), _bits(host))
    far = thousand + np.array([500.0, 500.0, 0.0, 0.0, 0.0, 0.0])
    assert not m.score_poses(*scan, _list(far)).cpu().numpy().any()
    assert m.best_poses(*scan, _list(far)) == [] and m.best_poses_align(*scan, _list(far)) == []


def test_a_list_searches_z_roll_and_pitch(matcher, small, scan):
    """What the (x, y, yaw) lattice cannot do: the golden final pose plus every combination of a z offset in
    {-0.4, -0.2, 0, 0.2, 0.4} and roll and pitch offsets in {-0.06, -0.03, 0, 0.03, 0.06}, 125 poses, shuffled.  Checked
    on the CPU with evaluate3(mirror32=True): the zero-offset pose scores 380.5, the runner-up (pitch +0.03) 231.7, the
    worst 70.6 - a margin far outside the float32 error."""
    c = np.asarray(small["pose"], dtype=np.float64)
    offs = list(itertools.product((-0.4, -0.2, 0.0, 0.2, 0.4), (-0.06, -0.03, 0.0, 0.03, 0.06), (-0.06, -0.03, 0.0, 0.03, 0.06)))
    poses = np.array([c + np.array([0.0, 0.0, dz, dr, dp, 0.0]) for dz, dr, dp in offs])
    perm = np.random.default_rng(7).permutation(len(poses))
    poses = poses[perm]
    want = int(np.flatnonzero(perm == offs.index((0.0, 0.0, 0.0)))[0])
    assert tuple(poses[want]) == small["pose"]
    hits = matcher.best_poses(*scan, _list(poses), k=1)
    assert len(hits) == 1 and hits[0].index == want and hits[0].pose == small["pose"]
    scores = matcher.score_poses(*scan, _list(poses)).cpu().numpy()
    print("best", scores[want], "runner-up", np.sort(scores)[-2], "worst", scores.min())


def test_errors_leave_the_handle_intact(gpu_lib, small, thousand):
    import torch
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = small
    lib = gpu_lib
    s = _dev(d["sx"], d["sy"], d["sz"])
    n = s[0].numel()
    dl = _list(thousand[:100])
    out = torch.zeros(100, dtype=torch.float32, device="cuda")
    hits = (L.SearchHit3D * 64)()
    res = (L.Result3D * 64)()
    nh = C.c_int32(-1)
    ptr = lambda t: None if t is None else t.data_ptr()

    def score(m, null=None, nn=n, p=dl, mm=100, o=out):
        return lib.ndt3d_score_poses_dev(m._h, *[None if a == null else ptr(t) for a, t in enumerate(s)], nn, ptr(p), mm, ptr(o))

    def best(m, null=None, nn=n, p=dl, mm=100, sep=(0.5, 0.1), k=8, hp=hits, np_=nh, align=False, rp=res):
        h = C.cast(hp, C.c_void_p) if hp is not None else None
        c = C.byref(np_) if np_ is not None else None
        sp = [None if a == null else ptr(t) for a, t in enumerate(s)]
        if align:
            return lib.ndt3d_best_poses_align_dev(m._h, *sp, nn, ptr(p), mm, sep[0], sep[1], k, h,
                                                  C.cast(rp, C.c_void_p) if rp is not None else None, c)
        return lib.ndt3d_best_poses_dev(m._h, *sp, nn, ptr(p), mm, sep[0], sep[1], k, h, c)

    with NdtMatcher3D() as fresh:
        assert score(fresh) == L.NDT_ERR_NO_TARGET and best(fresh) == L.NDT_ERR_NO_TARGET
        hx = np.zeros(100, np.float32)
        assert lib.ndt3d_score_poses(fresh._h, d["sx"].ctypes.data, d["sy"].ctypes.data, d["sz"].ctypes.data, n,
                                     thousand.ctypes.data, 100, hx.ctypes.data) == L.NDT_ERR_NO_TARGET
        fresh.set_target(d["tx"], d["ty"], d["tz"])
        ref1 = fresh.align(*s, d["init"])
    with NdtMatcher3D() as m:
        m.set_target(d["tx"], d["ty"], d["tz"])
        m.wait_stream()
        for kw in (dict(null=0), dict(null=1), dict(null=2), dict(p=None), dict(o=None), dict(nn=0), dict(nn=2 ** 31), dict(mm=0)):
            assert score(m, **kw) == L.NDT_ERR_INVALID_ARG, kw
        assert score(m, mm=2 ** 25 + 1) == L.NDT_ERR_CAPACITY
        for kw in (dict(null=2), dict(p=None), dict(hp=None), dict(np_=None), dict(nn=0), dict(mm=0), dict(k=0), dict(k=65),
                   dict(sep=(NAN, 0.1)), dict(sep=(0.5, INF)), dict(sep=(-0.5, 0.1)), dict(sep=(0.5, -0.1))):
            assert best(m, **kw) == L.NDT_ERR_INVALID_ARG, kw
            assert best(m, align=True, **kw) == L.NDT_ERR_INVALID_ARG, kw
        assert best(m, align=True, rp=None) == L.NDT_ERR_INVALID_ARG
        assert best(m, mm=2 ** 25 + 1) == L.NDT_ERR_CAPACITY
        assert not out.cpu().numpy().any()
        # after the errors the handle aligns as a fresh one does, bit for bit
        assert _same(m.align(*s, d["init"]), ref1)
        # a call between two alignments, and one issued while an asynchronous alignment is in flight
        assert score(m) == L.NDT_OK and out.cpu().numpy().max() > 10.0
        alone = _bits(out)
        assert best(m) == L.NDT_OK and nh.value > 0
        assert _same(m.align(*s, d["init"]), ref1)
        m.align_async(*s, d["init"])
        during = _bits(m.score_poses(*s, dl))
        assert _same(m.finish(), ref1)
        assert np.array_equal(during, alone)
        m.align_async(*s, d["init"])
        assert best(m) == L.NDT_OK and nh.value > 0
        assert _same(m.finish(), ref1)
    with NdtMatcher3D() as empty:
        empty.reserve_target((-10.0, -10.0, -3.0), (10.0, 10.0, 3.0))
        out.fill_(3.0)
        torch.cuda.synchronize()
        assert score(empty) == L.NDT_OK and not out.cpu().numpy().any()
        assert best(empty) == L.NDT_OK and nh.value == 0
