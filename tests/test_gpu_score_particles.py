"""The score and the hit count of a scan at a short list of poses, a team of lanes per pose (ndt2d_score_particles*):
against the float64 restatement (tests/score_poses_ref.py) and evaluate()'s n_hit, against the list kernel by the bound
that two sums of the same terms obey, bit for bit where the two orders coincide, independent of the team width and of
the list's shape, exact zeros for non-finite poses, the asynchronous form, and the errors.

The lists `near` and `thousand` are those of test_gpu_score_poses.py (the same seeds and spreads, restated)."""
import math

import numpy as np
import pytest

import score_poses_ref as R
from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import synth

pytestmark = pytest.mark.gpu

NAN, INF = math.nan, math.inf
TEAMS = (64, 256, 0)                                # the two widths and the default (by the list's length)


def _dev(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in arrays)


def _list(poses):
    import torch
    return torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3)).cuda()


def _bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return np.ascontiguousarray(a).view(np.uint32)


def _same(a, b):
    return (a.pose == b.pose and a.iterations == b.iterations and a.status == b.status and a.n_hit == b.n_hit
            and a.score == b.score and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g))


def _both(m, scan, poses, team=0):
    """(score bits, counts) as numpy uint32 arrays, with the team knob at `team` for the call."""
    m.set_tuning("particle_team", team)
    try:
        s, c = m.score_particles(*scan, poses if hasattr(poses, "data_ptr") else _list(poses), with_hits=True)
    finally:
        m.set_tuning("particle_team", 0)
    return _bits(s), _bits(c)


@pytest.fixture(scope="module")
def pair1():
    return synth.make_pair(1)


@pytest.fixture(scope="module")
def matchers(gpu_lib, pair1):
    """One handle per overlap_grids, each holding the fixture's target."""
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    with NdtMatcher2D() as m1, NdtMatcher2D(overlap_grids=4) as m4:
        for m in (m1, m4):
            m.set_target(pair1["tx"], pair1["ty"])
        yield {1: m1, 4: m4}


@pytest.fixture(scope="module")
def matcher(matchers):
    return matchers[1]


@pytest.fixture(scope="module")
def scan(pair1):
    return _dev(pair1["sx"], pair1["sy"])


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


def _oracle(pair1, sx, sy, poses, overlap):
    from oracle import ndt2d as o
    prm = o.NdtParams(overlap=overlap)
    return R.scores2d(o.build_grids(pair1["tx"], pair1["ty"], prm), sx, sy, poses, prm)


@pytest.mark.parametrize("overlap", [1, 4])
def test_scores_match_the_oracle_and_counts_match_evaluate(matchers, pair1, scan, near, overlap):
    m = matchers[overlap]
    ref = _oracle(pair1, pair1["sx"], pair1["sy"], near, overlap)
    dl = _list(near)
    got, hit = m.score_particles(*scan, dl, with_hits=True)
    got, hit = got.cpu().numpy(), hit.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (258,) and hit.dtype == np.uint32 and hit.shape == (258,)
    err = np.abs(got.astype(np.float64) - ref)
    print("largest error over the bound:", float(np.max(err - (1e-4 * np.abs(ref) + 1e-3))), "max ref", ref.max())
    assert np.all(err <= 1e-4 * np.abs(ref) + 1e-3)
    assert np.max(ref) > 10.0
    want = np.array([m.evaluate(*scan, tuple(p))[3] for p in near], dtype=np.uint32)
    assert np.array_equal(hit, want)
    assert want.max() > 500 and want.min() < want.max()
    assert np.array_equal(_bits(m.score_particles(*scan, dl)), _bits(got))           # with_hits=False: the same bits


@pytest.mark.parametrize("overlap", [1, 4])
def test_the_list_kernel_is_within_the_bound_of_two_summation_orders(matchers, scan, thousand, overlap):
    """Both sums add the same K = n * overlap_grids non-negative float32 terms, and any order of K terms lies within
    gamma_(K-1) of the exact sum: so the two differ by at most 2 gamma_(K-1) < 2.1 K 2^-24 relative."""
    m = matchers[overlap]
    dl = _list(thousand)
    lst = m.score_poses(*scan, dl).cpu().numpy().astype(np.float64)
    got = m.score_particles(*scan, dl).cpu().numpy().astype(np.float64)
    K = scan[0].numel() * overlap
    bound = 2.1 * K * 2.0 ** -24 * lst
    print("largest difference over the bound:", float(np.max(np.abs(got - lst) - bound)), "K", K)
    assert np.all(np.abs(got - lst) <= bound)
    assert np.count_nonzero(got > 0) > 900


@pytest.mark.parametrize("overlap", [1, 4])
@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_points_are_the_list_kernel_bit_for_bit(matchers, pair1, thousand, overlap, n):
    """n <= 2: both orders reduce to the same additions (the other partial sums are +0), so the bound is equality."""
    m = matchers[overlap]
    s = _dev(pair1["sx"][:n], pair1["sy"][:n])
    dl = _list(thousand[:300])
    lst = _bits(m.score_poses(*s, dl))
    for team in TEAMS:
        got, _ = _both(m, s, dl, team)
        assert np.array_equal(got, lst), team
    assert np.count_nonzero(lst.view(np.float32) > 0) >= 50


@pytest.mark.parametrize("overlap", [1, 4])
def test_the_team_width_never_changes_a_bit(matchers, pair1, thousand, overlap):
    m = matchers[overlap]
    dl = _list(thousand[:130])
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        s = _dev(pair1["sx"][:n], pair1["sy"][:n])
        got = [_both(m, s, dl, team) for team in TEAMS]
        for sc, cn in got[1:]:
            assert np.array_equal(sc, got[0][0]) and np.array_equal(cn, got[0][1]), n
        assert got[0][1].max() <= n * overlap
    assert np.count_nonzero(got[0][0]) > 100 and got[0][1].max() > 500


def test_a_score_does_not_depend_on_the_list(matcher, scan, thousand):
    import torch
    m = matcher
    full, cnt = _both(m, scan, thousand)
    again = _both(m, scan, thousand)
    assert np.array_equal(full, again[0]) and np.array_equal(cnt, again[1])            # two calls, the same bits
    assert np.count_nonzero(full) > 900 and np.count_nonzero(cnt) > 900
    for team in (64, 256):
        m.set_tuning("particle_team", team)
        for k in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1000):
            poses = _list(thousand[:k])
            out = torch.full((k + 64,), -7.0, dtype=torch.float32, device="cuda")
            hit = torch.full((k + 64,), -7, dtype=torch.int32, device="cuda")
            m.wait_stream()
            st = m._c.score_particles_dev(m._h, scan[0].data_ptr(), scan[1].data_ptr(), scan[0].numel(), poses.data_ptr(), k,
                                          out.data_ptr(), hit.data_ptr())
            assert st == L.NDT_OK
            out, hit = out.cpu().numpy(), hit.cpu().numpy()
            assert np.array_equal(out[:k].view(np.uint32), full[:k]), (team, k)
            assert np.array_equal(hit[:k].view(np.uint32), cnt[:k]), (team, k)
            assert np.all(out[k:] == -7.0) and np.all(hit[k:] == -7), (team, k)         # the guards are untouched
        # the tail of the list, so that an entry changes its workgroup and its wave; a fixed permutation
        tail = _both(m, scan, thousand[301:], team)
        assert np.array_equal(tail[0], full[301:]) and np.array_equal(tail[1], cnt[301:])
        perm = np.random.default_rng(5).permutation(1000)
        mixed = _both(m, scan, thousand[perm], team)
        assert np.array_equal(mixed[0], full[perm]) and np.array_equal(mixed[1], cnt[perm])
    m.set_tuning("particle_team", 0)


def test_nan_points_add_nothing(matcher, pair1, scan, near, thousand):
    """Appended NaN points keep every other point's virtual lane: the bits stay.  Spliced ones move the points behind
    them to other lanes, so the sum's order changes: those are held to the float64 restatement."""
    m = matcher
    dl = _list(thousand[:130])
    clean = _both(m, scan, dl)
    pad = np.full(300, NAN, np.float32)
    for team in TEAMS:
        for fill in ((pad, pad), (pad, np.zeros(300, np.float32)), (np.ones(300, np.float32), pad)):
            s = _dev(np.concatenate([pair1["sx"], fill[0]]), np.concatenate([pair1["sy"], fill[1]]))
            got = _both(m, s, dl, team)
            assert np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1]), team
    at = [0, 254, 254, 1000]                                       # np.insert: before these indices of the 1000-point scan
    sx, sy = np.insert(pair1["sx"], at, NAN), np.insert(pair1["sy"], at, [NAN, 0.5, NAN, NAN])
    assert sx.size == 1004 and np.flatnonzero(np.isnan(sx)).tolist() == [0, 255, 256, 1003]
    poses = near[-32:]
    ref = _oracle(pair1, sx, sy, poses, 1)
    assert np.max(ref) > 10.0
    want = np.array([m.evaluate(*scan, tuple(p))[3] for p in poses], dtype=np.uint32)
    for team in TEAMS:
        sc, cn = _both(m, _dev(sx, sy), poses, team)
        err = np.abs(sc.view(np.float32).astype(np.float64) - ref)
        assert np.all(err <= 1e-4 * np.abs(ref) + 1e-3), team
        assert np.array_equal(cn, want), team


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


def test_non_finite_poses_score_exactly_zero_with_count_zero(matcher, pair1, scan, thousand):
    m = matcher
    clean, clean_hit = _both(m, scan, thousand[:300])
    bad, idx = _poisoned(thousand)
    assert len(idx) == 10
    rest = np.setdiff1d(np.arange(300), idx)
    for team in (64, 256):
        got, hit = _both(m, scan, bad, team)
        assert np.all(got[idx] == 0) and np.all(hit[idx] == 0)            # +0.0f: all bits clear; count 0
        assert np.all(clean[idx] != 0) and np.all(clean_hit[idx] != 0)
        assert np.array_equal(got[rest], clean[rest]) and np.array_equal(hit[rest], clean_hit[rest])
    host, host_hit = m.score_particles(pair1["sx"], pair1["sy"], bad, with_hits=True)
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and host_hit.dtype == np.uint32
    assert np.array_equal(_bits(host), got) and np.array_equal(host_hit, hit)
    assert np.array_equal(_bits(m.score_particles(pair1["sx"], pair1["sy"], bad)), got)


def test_finite_poses_beyond_float32_score_exactly_zero(matcher, scan, thousand):
    m = matcher
    clean, clean_hit = _both(m, scan, thousand[:130])
    bad = thousand[:130].copy()
    absurd = {0: (0, 1e300), 63: (1, -1e39), 64: (2, 1e300), 65: (2, -1.7e308), 129: (2, 1e19)}
    for i, (coord, v) in absurd.items():
        bad[i, coord] = v
    rest = np.setdiff1d(np.arange(130), sorted(absurd))
    for team in (64, 256):
        got, hit = _both(m, scan, bad, team)
        val = got.view(np.float32)
        assert np.isfinite(val).all() and np.all(val >= 0.0)             # whatever an absurd heading wraps to: never NaN
        assert np.all(got[[0, 63]] == 0) and np.all(hit[[0, 63]] == 0)   # the translations beyond float32: +0.0f
        assert np.array_equal(got[rest], clean[rest]) and np.array_equal(hit[rest], clean_hit[rest])


def test_the_asynchronous_form(matcher, pair1, scan, thousand):
    import torch
    m = matcher
    dl = _list(thousand)
    ref, ref_hit = m.score_particles(*scan, dl, with_hits=True)
    want_sum, want_hits = ref.sum(), ref_hit.view(torch.int32).sum()
    # consumed on torch's current stream, with no synchronisation between the call and the reduction
    got, hit = m.score_particles(*scan, dl, with_hits=True, sync=False)
    same = (got.view(torch.int32) == ref.view(torch.int32)).all() & (hit.view(torch.int32) == ref_hit.view(torch.int32)).all()
    total, total_hits = got.sum(), hit.view(torch.int32).sum()
    assert bool(same) and float(total) == float(want_sum) and int(total_hits) == int(want_hits)
    only = m.score_particles(*scan, dl, sync=False)
    assert bool((only.view(torch.int32) == ref.view(torch.int32)).all())
    with pytest.raises(ValueError):
        m.score_particles(pair1["sx"], pair1["sy"], thousand, sync=False)
    # issued while an asynchronous alignment is in flight: the same bits, and the alignment bit for bit as alone
    alone = m.align(*scan, pair1["init"])
    for sync in (True, False):
        m.align_async(*scan, pair1["init"])
        got, hit = m.score_particles(*scan, dl, with_hits=True, sync=sync)
        during = _bits(got), _bits(hit)
        assert _same(m.finish(), alone)
        assert np.array_equal(during[0], _bits(ref)) and np.array_equal(during[1], _bits(ref_hit))


def test_errors_leave_the_handle_intact(gpu_lib, pair1, thousand):
    import torch
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = pair1
    lib = gpu_lib
    sx, sy = _dev(d["sx"], d["sy"])
    n = sx.numel()
    dl = _list(thousand[:100])
    out = torch.zeros(100, dtype=torch.float32, device="cuda")
    hit = torch.zeros(100, dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    hx, hn = np.zeros(100, np.float32), np.zeros(100, np.uint32)

    def dev(m, x=sx, y=sy, nn=n, p=dl, mm=100, o=out, c=hit, fn=lib.ndt2d_score_particles_dev):
        return fn(m._h, ptr(x), ptr(y), nn, ptr(p), mm, ptr(o), ptr(c))

    def asy(m, **kw):
        return dev(m, fn=lib.ndt2d_score_particles_async, **kw)

    def host(m, x=d["sx"], y=d["sy"], nn=n, p=thousand, mm=100, o=hx, c=hn):
        a = lambda v: None if v is None else v.ctypes.data
        return lib.ndt2d_score_particles(m._h, a(x), a(y), nn, a(p), mm, a(o), a(c))

    with NdtMatcher2D() as fresh:
        for call in (dev, asy, host):
            assert call(fresh) == L.NDT_ERR_NO_TARGET, call.__name__
        fresh.set_target(d["tx"], d["ty"])
        ref1 = fresh.align(sx, sy, d["init"])
    with NdtMatcher2D() as m:
        m.set_target(d["tx"], d["ty"])
        m.wait_stream()
        for call in (dev, asy, host):
            for kw in (dict(x=None), dict(y=None), dict(p=None), dict(o=None), dict(nn=0), dict(nn=2 ** 31), dict(mm=0)):
                assert call(m, **kw) == L.NDT_ERR_INVALID_ARG, (call.__name__, kw)
            assert call(m, mm=2 ** 25 + 1) == L.NDT_ERR_CAPACITY, call.__name__
        for v in (-1, 1, 32, 63, 65, 128, 255, 257, 512, 1024):
            assert lib.ndt2d_set_tuning(m._h, L.TUNING["particle_team"], v) == L.NDT_ERR_INVALID_ARG, v
        for v in (64, 256, 0):
            assert lib.ndt2d_set_tuning(m._h, L.TUNING["particle_team"], v) == L.NDT_OK, v
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any() and not hit.cpu().numpy().any() and not hx.any() and not hn.any()
        # after the errors the handle aligns as a fresh one does, bit for bit
        assert _same(m.align(sx, sy, d["init"]), ref1)
        # a null count pointer is accepted, and the scores are the same
        assert dev(m) == L.NDT_OK and out.cpu().numpy().max() > 10.0 and hit.cpu().numpy().max() > 500
        with_counts = _bits(out)
        out.zero_()
        torch.cuda.synchronize()
        assert dev(m, c=None) == L.NDT_OK and np.array_equal(_bits(out), with_counts)
        out.zero_()
        torch.cuda.synchronize()
        assert asy(m, c=None) == L.NDT_OK
        torch.cuda.current_stream().wait_stream(torch.cuda.ExternalStream(m.stream))
        assert np.array_equal(_bits(out), with_counts)
        assert host(m, c=None) == L.NDT_OK and np.array_equal(hx.view(np.uint32), with_counts)
        assert host(m) == L.NDT_OK and np.array_equal(hn, hit.cpu().numpy().view(np.uint32))
        assert _same(m.align(sx, sy, d["init"]), ref1)
    with NdtMatcher2D() as empty:
        empty.reserve_target(-10.0, -10.0, 10.0, 10.0)
        out.fill_(3.0)
        hit.fill_(3)
        torch.cuda.synchronize()
        assert dev(empty) == L.NDT_OK and not out.cpu().numpy().any() and not hit.cpu().numpy().any()
