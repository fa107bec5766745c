"""The score and the hit count of a scan at a short list of 3D poses, a team of lanes per pose (ndt3d_score_particles*):
against oracle.ndt3d.evaluate3(mirror32=True) (tests/score_poses_ref.py) and evaluate()'s n_hit, against the list kernel
by the bound that two sums of the same terms obey, bit for bit where the two orders coincide, independent of the team
width and of the list's shape, exact zeros for non-finite poses, the asynchronous form, and the errors.

The lists `near` and `thousand` are those of test_gpu_score_poses3d.py (the same seeds and spreads, restated)."""
import itertools
import math
import os

import numpy as np
import pytest

import score_poses_ref as R
from gtsam_ndt_amd import _lib as L

pytestmark = pytest.mark.gpu

NAN, INF = math.nan, math.inf
GOLD3 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ndt3d_small.npz")
TEAMS = (64, 256, 0)                                # the two widths and the default (by the list's length)


def _dev(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in arrays)


def _list(poses):
    import torch
    return torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 6)).cuda()


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


def _oracle(small, sx, sy, sz, poses):
    from oracle import ndt3d as o
    prm = o.Ndt3Params()
    return R.scores3d(o.build_grid3(small["tx"], small["ty"], small["tz"], prm), sx, sy, sz, poses, prm)


def test_scores_match_the_oracle_and_counts_match_evaluate(matcher, small, scan, near):
    m = matcher
    ref = _oracle(small, small["sx"], small["sy"], small["sz"], near)
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


def test_the_list_kernel_is_within_the_bound_of_two_summation_orders(matcher, scan, thousand):
    """Both sums add the same K = n non-negative float32 terms, and any order of K terms lies within gamma_(K-1) of the
    exact sum: so the two differ by at most 2 gamma_(K-1) < 2.1 K 2^-24 relative."""
    m = matcher
    dl = _list(thousand)
    lst = m.score_poses(*scan, dl).cpu().numpy().astype(np.float64)
    got = m.score_particles(*scan, dl).cpu().numpy().astype(np.float64)
    K = scan[0].numel()
    bound = 2.1 * K * 2.0 ** -24 * lst
    print("largest difference over the bound:", float(np.max(np.abs(got - lst) - bound)), "K", K)
    assert np.all(np.abs(got - lst) <= bound)
    assert np.count_nonzero(got > 0) > 900


@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_points_are_the_list_kernel_bit_for_bit(matcher, small, thousand, n):
    """n <= 2: both orders reduce to the same additions (the other partial sums are +0), so the bound is equality."""
    m = matcher
    s = _dev(small["sx"][:n], small["sy"][:n], small["sz"][:n])
    dl = _list(thousand[:200])
    lst = _bits(m.score_poses(*s, dl))
    for team in TEAMS:
        got, _ = _both(m, s, dl, team)
        assert np.array_equal(got, lst), team
    assert np.count_nonzero(lst.view(np.float32) > 0) >= 50


def test_the_team_width_never_changes_a_bit(matcher, small, thousand):
    m = matcher
    dl = _list(thousand[:130])
    for n in (1, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 4096):
        s = _dev(small["sx"][:n], small["sy"][:n], small["sz"][:n])
        got = [_both(m, s, dl, team) for team in TEAMS]
        for sc, cn in got[1:]:
            assert np.array_equal(sc, got[0][0]) and np.array_equal(cn, got[0][1]), n
        assert got[0][1].max() <= n
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
            st = m._c.score_particles_dev(m._h, *[a.data_ptr() for a in scan], scan[0].numel(), poses.data_ptr(), k,
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


def test_nan_points_add_nothing(matcher, small, scan, near, thousand):
    """Appended NaN points keep every other point's virtual lane: the bits stay.  Spliced ones move the points behind
    them to other lanes, so the sum's order changes: those are held to the float64 restatement."""
    m = matcher
    cloud = [small["sx"], small["sy"], small["sz"]]
    dl = _list(thousand[:130])
    clean = _both(m, scan, dl)
    pad, one = np.full(300, NAN, np.float32), np.ones(300, np.float32)
    for team in TEAMS:
        for fill in ((pad, pad, pad), (pad, one, one), (one, pad, one), (one, one, pad)):
            s = _dev(*(np.concatenate([a, f]) for a, f in zip(cloud, fill)))
            got = _both(m, s, dl, team)
            assert np.array_equal(got[0], clean[0]) and np.array_equal(got[1], clean[1]), team
    at = [0, 254, 254, 4096]                                       # np.insert: before these indices of the 4096-point scan
    vals = ([NAN, NAN, 1.0, NAN], [NAN, 1.0, NAN, NAN], [NAN, 1.0, 1.0, NAN])
    spliced = [np.insert(a, at, v).astype(np.float32) for a, v in zip(cloud, vals)]
    bad = np.isnan(spliced[0]) | np.isnan(spliced[1]) | np.isnan(spliced[2])
    assert spliced[0].size == 4100 and np.flatnonzero(bad).tolist() == [0, 255, 256, 4099]
    poses = near[-32:]
    ref = _oracle(small, *spliced, poses)
    assert np.max(ref) > 10.0
    want = np.array([m.evaluate(*scan, tuple(p))[3] for p in poses], dtype=np.uint32)
    for team in TEAMS:
        sc, cn = _both(m, _dev(*spliced), poses, team)
        err = np.abs(sc.view(np.float32).astype(np.float64) - ref)
        assert np.all(err <= 1e-4 * np.abs(ref) + 1e-3), team
        assert np.array_equal(cn, want), team


def test_non_finite_poses_score_exactly_zero_with_count_zero(matcher, small, scan, thousand):
    m = matcher
    clean, clean_hit = _both(m, scan, thousand[:300])
    bad = thousand[:300].copy()
    idx = [0, 1, 2, 62, 63, 64, 65, 66, 67, 128, 129, 130, 254, 255, 256, 257, 298, 299]
    for i, (coord, v) in zip(idx, itertools.product(range(6), (NAN, INF, -INF))):
        bad[i, coord] = v
    rest = np.setdiff1d(np.arange(300), idx)
    for team in (64, 256):
        got, hit = _both(m, scan, bad, team)
        assert np.all(got[idx] == 0) and np.all(hit[idx] == 0)            # +0.0f: all bits clear; count 0
        assert np.all(clean[idx] != 0) and np.all(clean_hit[idx] != 0)
        assert np.array_equal(got[rest], clean[rest]) and np.array_equal(hit[rest], clean_hit[rest])
    host, host_hit = m.score_particles(small["sx"], small["sy"], small["sz"], bad, with_hits=True)
    assert isinstance(host, np.ndarray) and host.dtype == np.float32 and host_hit.dtype == np.uint32
    assert np.array_equal(_bits(host), got) and np.array_equal(host_hit, hit)
    assert np.array_equal(_bits(m.score_particles(small["sx"], small["sy"], small["sz"], bad)), got)


def test_finite_poses_beyond_float32_score_exactly_zero(matcher, scan, thousand):
    m = matcher
    clean, clean_hit = _both(m, scan, thousand[:130])
    bad = thousand[:130].copy()
    absurd = {0: (0, 1e300), 1: (2, 1e39), 63: (1, -1e39), 64: (3, 1e300), 65: (4, -1.7e308), 129: (5, 1e19)}
    for i, (coord, v) in absurd.items():
        bad[i, coord] = v
    rest = np.setdiff1d(np.arange(130), sorted(absurd))
    for team in (64, 256):
        got, hit = _both(m, scan, bad, team)
        val = got.view(np.float32)
        assert np.isfinite(val).all() and np.all(val >= 0.0)             # whatever an absurd angle wraps to: never NaN
        assert np.all(got[[0, 1, 63]] == 0) and np.all(hit[[0, 1, 63]] == 0)   # the translations beyond float32: +0.0f
        assert np.array_equal(got[rest], clean[rest]) and np.array_equal(hit[rest], clean_hit[rest])


def test_the_asynchronous_form(matcher, small, scan, thousand):
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
        m.score_particles(small["sx"], small["sy"], small["sz"], thousand, sync=False)
    # issued while an asynchronous alignment is in flight: the same bits, and the alignment bit for bit as alone
    alone = m.align(*scan, small["init"])
    for sync in (True, False):
        m.align_async(*scan, small["init"])
        got, hit = m.score_particles(*scan, dl, with_hits=True, sync=sync)
        during = _bits(got), _bits(hit)
        assert _same(m.finish(), alone)
        assert np.array_equal(during[0], _bits(ref)) and np.array_equal(during[1], _bits(ref_hit))


def test_errors_leave_the_handle_intact(gpu_lib, small, thousand):
    import torch
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = small
    lib = gpu_lib
    s = _dev(d["sx"], d["sy"], d["sz"])
    hs = (d["sx"], d["sy"], d["sz"])
    n = s[0].numel()
    dl = _list(thousand[:100])
    out = torch.zeros(100, dtype=torch.float32, device="cuda")
    hit = torch.zeros(100, dtype=torch.int32, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    hx, hn = np.zeros(100, np.float32), np.zeros(100, np.uint32)

    def dev(m, null=None, nn=n, p=dl, mm=100, o=out, c=hit, fn=lib.ndt3d_score_particles_dev):
        return fn(m._h, *[None if a == null else ptr(t) for a, t in enumerate(s)], nn, ptr(p), mm, ptr(o), ptr(c))

    def asy(m, **kw):
        return dev(m, fn=lib.ndt3d_score_particles_async, **kw)

    def host(m, null=None, nn=n, p=thousand, mm=100, o=hx, c=hn):
        a = lambda v: None if v is None else v.ctypes.data
        return lib.ndt3d_score_particles(m._h, *[None if i == null else a(t) for i, t in enumerate(hs)], nn, a(p), mm, a(o), a(c))

    with NdtMatcher3D() as fresh:
        for call in (dev, asy, host):
            assert call(fresh) == L.NDT_ERR_NO_TARGET, call.__name__
        fresh.set_target(d["tx"], d["ty"], d["tz"])
        ref1 = fresh.align(*s, d["init"])
    with NdtMatcher3D() as m:
        m.set_target(d["tx"], d["ty"], d["tz"])
        m.wait_stream()
        for call in (dev, asy, host):
            for kw in (dict(null=0), dict(null=1), dict(null=2), dict(p=None), dict(o=None), dict(nn=0), dict(nn=2 ** 31),
                       dict(mm=0)):
                assert call(m, **kw) == L.NDT_ERR_INVALID_ARG, (call.__name__, kw)
            assert call(m, mm=2 ** 25 + 1) == L.NDT_ERR_CAPACITY, call.__name__
        for v in (-1, 1, 32, 63, 65, 128, 255, 257, 512, 1024):
            assert lib.ndt3d_set_tuning(m._h, L.TUNING["particle_team"], v) == L.NDT_ERR_INVALID_ARG, v
        for v in (64, 256, 0):
            assert lib.ndt3d_set_tuning(m._h, L.TUNING["particle_team"], v) == L.NDT_OK, v
        torch.cuda.synchronize()
        assert not out.cpu().numpy().any() and not hit.cpu().numpy().any() and not hx.any() and not hn.any()
        # after the errors the handle aligns as a fresh one does, bit for bit
        assert _same(m.align(*s, d["init"]), ref1)
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
        assert _same(m.align(*s, d["init"]), ref1)
    with NdtMatcher3D() as empty:
        empty.reserve_target((-10.0, -10.0, -3.0), (10.0, 10.0, 3.0))
        out.fill_(3.0)
        hit.fill_(3)
        torch.cuda.synchronize()
        assert dev(empty) == L.NDT_OK and not out.cpu().numpy().any() and not hit.cpu().numpy().any()
