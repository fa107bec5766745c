"""ndt3d_align_map_multi: up to 64 3D map-to-map alignments against one target in one launch chain (docs/ALGORITHM.md
section 2.16a).  Every comparison is bitwise against ndt3d_align_map on the same handles from the same pose (_same is
that of tests/test_gpu_d2d3.py): there is no tolerance to choose.

Scenes (those of tests/test_gpu_d2d3.py).  Component counts by tests/d2d3_ref.py: "near1m" source 2214 / target 2706
(9 and 11 workgroups of 256), its crop to |x|, |y| < 6 m 141 (one workgroup); "stock2m" source 657 / target 817 (3 and 4),
crop 37.  The block of test 3 has 48 x 48 x 30 = 69 120 valid voxels: the cap of 256 workgroups is reached and every
lane walks the list in strides of 65 536."""
import ctypes as C
import math

import numpy as np
import pytest

from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import search, synth3d
from oracle import ndt3d as O

pytestmark = pytest.mark.gpu

POSE_A = (0.10, -0.08, 0.02, 0.004, -0.003, 0.01)
SCENES = {"near1m": (POSE_A, 1.0), "stock2m": (None, 2.0)}
# max_iterations = 20: ndt3d_align_map from the starts near the zero guess converges in 6 to 15 iterations on these scenes
# in either Hessian form, the starts metres off take up to the default cap of 100: some starts of a call end by
# themselves and the others at the cap
VARIANTS = {
    "converged": dict(),
    "converged_linesearch4": dict(line_search=4),
    "fixed7": dict(fixed_iterations=7),
    "cut20_relaxed1.5": dict(max_iterations=20, step_scale=1.5),
}
ZERO = (0.0,) * 6
BLOCK, MAX_BLOCKS = 256, 256
CROP = 6.0
BOX = ((-22.0, -22.0, -3.0), (22.0, 22.0, 6.0))
DEG = math.pi / 180.0
_cache = {}


def _pair(scene):
    pose = SCENES[scene][0]
    if pose not in _cache:
        _cache[pose] = synth3d.make_pair3d(pose=pose) if pose is not None else synth3d.make_pair3d()
    return _cache[pose]


def _same(a, b):
    return (a.pose == b.pose and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g) and a.score == b.score and
            a.iterations == b.iterations and a.n_hit == b.n_hit and a.status == b.status)


def _matcher(x, y, z, **kw):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    m = NdtMatcher3D(**kw)
    m.set_target(x, y, z)
    return m


def _handles(scene, **kw):
    d = _pair(scene)
    kw.setdefault("cell_size", SCENES[scene][1])
    return _matcher(d["tx"], d["ty"], d["tz"], **kw), _matcher(d["sx"], d["sy"], d["sz"], **kw)


def _cropped(scene, **kw):
    d = _pair(scene)
    kw.setdefault("cell_size", SCENES[scene][1])
    k = (np.abs(d["sx"]) < CROP) & (np.abs(d["sy"]) < CROP)
    return _matcher(d["sx"][k], d["sy"][k], d["sz"][k], **kw)


def _blocks(n):
    return min((n + BLOCK - 1) // BLOCK, MAX_BLOCKS)


def _spread(m):
    """The zero guess, then a deterministic spread around it (within 0.1 m / 0.04 rad: the basin of the generating
    poses); every fourth start is metres and a fraction of a radian off and every sixteenth lies off the target's grid,
    so that starts end at different iterations, at the iteration cap or with NDT_TOO_FEW_*."""
    out = []
    for k in range(m):
        p = [0.05 * ((7 * k) % 5 - 2), 0.04 * ((3 * k) % 7 - 3), 0.02 * ((5 * k) % 3 - 1),
             0.004 * ((2 * k) % 5 - 2), 0.003 * ((3 * k) % 5 - 2), 0.01 * ((5 * k) % 9 - 4)]
        if k == 0:
            p = [0.0] * 6
        if k % 4 == 3:
            far = (2.5, -1.5, 0.3, 0.05, -0.04, 0.3 * (1 + k // 16))
            p = [a + b for a, b in zip(p, far)]
        if k % 16 == 2:                               # off the target's grid: no component hits a voxel
            p[0] += 300.0
        out.append(tuple(p))
    return out


def _check(t, sources, poses, tag=""):
    """one multi call against the single calls from the same poses; returns the multi results"""
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    srcs = [sources] * len(poses) if isinstance(sources, NdtMatcher3D) else list(sources)
    multi = t.align_map_multi(sources, poses)
    assert len(multi) == len(poses)
    for k, (s, p, r) in enumerate(zip(srcs, poses, multi)):
        single = t.align_map(s, p)
        assert _same(r, single), (tag, k, p, r, single)
    return multi


# ---------------------------------------------------------------------------------------------- 1. multi-start identity
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_every_start_equals_its_single_alignment(gpu_lib, scene, mode, variant):
    t, s = _handles(scene, hessian_mode=mode, **VARIANTS[variant])
    try:
        t.set_tuning("map_multi_from", 1)             # m = 1 takes the chain as well
        poses = _spread(64)
        single = [t.align_map(s, p) for p in poses]
        for m in (1, 2, 3, 5, 16, 64):
            multi = t.align_map_multi(s, poses[:m])
            assert len(multi) == m
            for k in range(m):
                assert _same(multi[k], single[k]), (m, k, poses[k], multi[k], single[k])
        its = sorted({r.iterations for r in single})
        sts = sorted({r.status for r in single})
        print(f"{scene} mode {mode} {variant}: iteration counts {its}, statuses {sts}")
        if "fixed" not in variant:                    # (a fixed run ends every start at the same launch by construction)
            assert len(its) >= 2                      # starts finish at different launches: the freezing is exercised
    finally:
        t.close(); s.close()


# ---------------------------------------------------------------------------------------------- 2. mixed sources
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_mixed_sources_in_one_call(gpu_lib, scene, mode):
    kw = dict(hessian_mode=mode)
    t, full = _handles(scene, **kw)
    crop = _cropped(scene, **kw)
    try:
        counts = {name: h.components()[0].size for name, h in (("full", full), ("crop", crop), ("target", t))}
        blocks = {name: _blocks(c) for name, c in counts.items()}
        print(f"{scene}: components {counts}, blocks {blocks}")
        assert 0 < counts["crop"] < BLOCK and blocks["full"] > 1 and blocks["target"] > 1
        near = (0.03, -0.02, 0.01, 0.002, -0.001, 0.004)
        # the one-workgroup list in slot 0, the widest (the target itself) in slot 2, one handle repeated
        sources = [crop, full, t, full, crop, full, t]
        poses = [ZERO, ZERO, ZERO, near, near, (-0.04, 0.03, 0.0, 0.0, 0.002, -0.01), near]
        _check(t, sources, poses, scene)
        _check(t, [crop, full], [near, ZERO], scene)          # the narrow list first and alone in a wide launch
        t.set_tuning("map_multi_from", 1)
        _check(t, [full], [near], scene)
        _check(t, [crop], [near], scene)
    finally:
        for h in (t, full, crop):
            h.close()


# ---------------------------------------------------------------------------------------------- 3. more than 65 536 components
def test_more_components_than_one_pass_of_the_launch(gpu_lib):
    """blocks capped at 256 workgroups: every lane walks the list in strides of 65 536 components."""
    rng = np.random.default_rng(20241018)
    nx, ny, nz, per = 48, 48, 30, 8
    ix, iy, iz = (a.ravel() for a in np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"))
    x, y, z = ((np.repeat(i, per) + rng.uniform(0.02, 0.98, i.size * per)).astype(np.float32) for i in (ix, iy, iz))
    assert x.size == 552_960
    big = _matcher(x, y, z, cell_size=1.0, fixed_iterations=3)
    try:
        n_comp = big.components()[0].size
        print(f"{n_comp} components")
        assert n_comp > 65536
        poses = [(0.05, -0.03, 0.02, 0.001, -0.002, 0.002), (-0.04, 0.06, -0.01, -0.002, 0.001, -0.003)]
        multi = _check(big, big, poses)
        assert all(r.iterations == 3 and r.n_hit > 0 for r in multi)
    finally:
        big.close()


# ---------------------------------------------------------------------------------------------- 4. empty participants
def test_empty_participants(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = _pair("near1m")
    t, s = _handles("near1m")
    off = (0.05, -0.04, 0.01, 0.002, -0.001, 0.01)
    far = (0.3, -0.2, 0.1, 0.0, 0.0, 0.05)
    try:
        with NdtMatcher3D() as hollow, NdtMatcher3D(min_points=100_000) as sparse:
            hollow.reserve_target(*BOX)                                  # a grid that never saw a point
            assert hollow.components()[0].size == 0
            for order in ([s, hollow, s], [hollow, s, s], [s, s, hollow]):
                poses = [ZERO, off, far]
                multi = t.align_map_multi(order, poses)
                for h, p, r in zip(order, poses, multi):
                    if h is hollow:
                        assert r.status == O.NDT_TOO_FEW_CELLS and r.pose == p and r.iterations == 0 and r.n_hit == 0
                        assert not r.H.any() and not r.g.any() and r.score == 0.0
                    else:
                        assert _same(r, t.align_map(s, p))
            only = t.align_map_multi([hollow, hollow], [ZERO, off])
            assert [r.status for r in only] == [O.NDT_TOO_FEW_CELLS] * 2 and [r.pose for r in only] == [ZERO, off]
            # a target without a valid voxel: every start
            sparse.set_target(d["tx"], d["ty"], d["tz"])
            multi = sparse.align_map_multi([s, t, s], [ZERO, off, ZERO])
            for p, r in zip([ZERO, off, ZERO], multi):
                assert r.status == O.NDT_TOO_FEW_CELLS and r.pose == p and r.iterations == 0 and r.n_hit == 0
            # and the handles go on as before
            _check(t, s, [ZERO, off])
    finally:
        t.close(); s.close()


# ---------------------------------------------------------------------------------------------- 5. dirty partial tables
def test_dirty_partial_tables(gpu_lib):
    """The multi-scan chain in Newton mode writes all 256 columns of 40 rows of every start's partial table; the map chain
    folds 32 rows x 256 columns of it and writes blocks[h] columns."""
    import torch
    d = _pair("near1m")
    kw = dict(hessian_mode=1)
    t, s = _handles("near1m", **kw)
    fresh_t, fresh_s = _handles("near1m", **kw)
    crop = _cropped("near1m", **kw)
    try:
        scan = tuple(torch.from_numpy(d["s" + a]).cuda() for a in "xyz")
        starts = _spread(64)
        poses = _spread(9)
        want_map = fresh_t.align_map_multi(fresh_s, poses)        # a handle whose multi context never held anything
        p2m = t.align_multi_scan([scan] * 64, starts)             # a fresh handle's answer; every column is dirty now
        got_map = t.align_map_multi(s, poses)
        assert all(_same(a, b) for a, b in zip(got_map, want_map))
        p2m_again = t.align_multi_scan([scan] * 64, starts)
        assert all(_same(a, b) for a, b in zip(p2m, p2m_again))
        again = t.align_map_multi(s, poses)                       # directly behind the point-to-map chain
        assert all(_same(a, b) for a, b in zip(again, want_map))
        for k, p in enumerate(poses):
            assert _same(want_map[k], t.align_map(s, p)), k
        # a wide start, then a one-workgroup start in the same slot
        t.set_tuning("map_multi_from", 1)
        fresh_t.set_tuning("map_multi_from", 1)
        near = poses[1]
        t.align_map_multi([s], [near])
        narrow = t.align_map_multi([crop], [near])[0]
        assert _same(narrow, t.align_map(crop, near))
        assert _same(narrow, fresh_t.align_map(crop, near))
        t.align_map_multi([s, t], [near, near])
        both = t.align_map_multi([crop, crop], [near, ZERO])
        assert _same(both[0], narrow) and _same(both[1], t.align_map(crop, ZERO))
    finally:
        for h in (t, s, fresh_t, fresh_s, crop):
            h.close()


# ---------------------------------------------------------------------------------------------- 6. the knob
def test_the_knob_changes_no_bit(gpu_lib):
    lib = gpu_lib
    t, s = _handles("near1m")
    try:
        poses = _spread(5)
        want = [t.align_map(s, p) for p in poses]
        for knob in (1, 2, 65):
            t.set_tuning("map_multi_from", knob)
            for m in (1, 2, 5):
                got = t.align_map_multi(s, poses[:m])
                assert len(got) == m and all(_same(a, b) for a, b in zip(got, want)), (knob, m)
        for bad in (0, 66):
            assert lib.ndt3d_set_tuning(t._h, L.TUNING["map_multi_from"], bad) == L.NDT_ERR_INVALID_ARG
        # every other knob keeps its answer
        assert lib.ndt3d_set_tuning(t._h, L.TUNING["single_sync_build"], 0) == L.NDT_OK
        assert lib.ndt3d_set_tuning(t._h, L.TUNING["single_sync_build"], 1) == L.NDT_OK
        assert lib.ndt3d_set_tuning(t._h, L.TUNING["launch_graphs"], 1) == L.NDT_ERR_INVALID_ARG
        assert lib.ndt3d_set_tuning(None, L.TUNING["map_multi_from"], 2) == L.NDT_ERR_INVALID_ARG
        got = t.align_map_multi(s, poses)             # the refused values left the knob at 65
        assert all(_same(a, b) for a, b in zip(got, want))
    finally:
        t.close(); s.close()


# ---------------------------------------------------------------------------------------------- 7. the caches
def test_derived_data_follows_the_grid(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    d = _pair("near1m")
    n = d["sx"].size
    first, second = np.arange(n // 2), np.arange(n // 2, n)
    poses = _spread(4)
    with NdtMatcher3D() as t, NdtMatcher3D() as s, NdtMatcher3D() as s2, NdtMatcher3D() as fixed_src:
        t.set_target(d["tx"], d["ty"], d["tz"])
        fixed_src.set_target(d["sx"], d["sy"], d["sz"])
        s.reserve_target(*BOX)
        s.add_target_points(d["sx"][first], d["sy"][first], d["sz"][first])
        sources = [s, fixed_src, s, s]
        before = t.align_map_multi(sources, poses)
        s.add_target_points(d["sx"][second], d["sy"][second], d["sz"][second])
        after = _check(t, sources, poses)                     # fresh single calls on the grown grid
        assert not _same(before[0], after[0]) and _same(before[1], after[1])
        s2.reserve_target(*BOX)
        s2.add_target_points(d["sx"], d["sy"], d["sz"])
        fresh = t.align_map_multi([s2, fixed_src, s2, s2], poses)
        assert all(_same(a, b) for a, b in zip(after, fresh))


# ---------------------------------------------------------------------------------------------- 8. the error table
def test_error_table_leaves_the_handles_intact(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    lib = gpu_lib
    d = _pair("near1m")
    with NdtMatcher3D() as t, NdtMatcher3D() as s, NdtMatcher3D() as empty:
        t.set_target(d["tx"], d["ty"], d["tz"])
        s.set_target(d["sx"], d["sy"], d["sz"])
        good_poses = _spread(3)
        want = _check(t, s, good_poses)

        def intact():
            got = t.align_map_multi(s, good_poses)
            assert all(_same(a, b) for a, b in zip(got, want))
            assert _same(s.align_map_multi(t, [ZERO])[0], s.align_map(t, ZERO))

        res = (L.Result3D * 64)()
        rp = C.cast(res, C.c_void_p)
        poses = (C.c_double * 18)(*[v for p in good_poses for v in p])

        def call(target, sources, p=poses, m=3, r=rp):
            hs = None if sources is None else (C.c_void_p * 64)(*[h._h.value if h is not None else None for h in sources])
            return lib.ndt3d_align_map_multi(target._h if target is not None else None, hs, p, m, r)

        assert call(t, [s, s, s]) == L.NDT_OK
        # null pointers, a null entry, m out of range
        assert call(None, [s, s, s]) == L.NDT_ERR_INVALID_ARG
        assert call(t, None) == L.NDT_ERR_INVALID_ARG
        assert call(t, [s, s, s], p=None) == L.NDT_ERR_INVALID_ARG
        assert call(t, [s, s, s], r=None) == L.NDT_ERR_INVALID_ARG
        assert call(t, [s, None, s]) == L.NDT_ERR_INVALID_ARG
        big = (C.c_double * (6 * 65))()
        for m in (0, 65, -1):
            assert call(t, [s] * 64, p=big, m=m) == L.NDT_ERR_INVALID_ARG
        intact()
        # a non-finite pose, in any start
        for bad in (float("nan"), float("inf"), -float("inf")):
            for j in range(18):
                p = (C.c_double * 18)(*poses)
                p[j] = bad
                assert call(t, [s, s, s], p=p) == L.NDT_ERR_INVALID_ARG
        intact()
        # a handle without a grid
        for target, sources in ((empty, [s, s, s]), (t, [s, empty, s]), (t, [empty, empty, empty])):
            assert call(target, sources) == L.NDT_ERR_NO_TARGET
        intact()
        # the Python wrapper: one pose per source
        with pytest.raises(ValueError):
            t.align_map_multi([s, s], good_poses)
        with pytest.raises(L.NdtError):
            t.align_map_multi(s, [ZERO] * 65)
        intact()


# ---------------------------------------------------------------------------------------------- 9. search_align_map
def test_search_align_map_refines_through_the_multi_call(gpu_lib):
    """The scene and the window of tests/test_gpu_search_map3d.py (its loop closure)."""
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    pose = (2.0, -1.5, 0.02, 0.004, -0.003, 0.6)
    offset = (1.6, -1.3, 0.0, 0.0, 0.0, 0.5)
    d = synth3d.make_pair3d(n_elev=32, n_azim=1024, pose=pose)
    guess = tuple(a + b for a, b in zip(pose, offset))
    window = search.Window(guess, (3.0, 3.0, math.pi), (0.5, 0.5, 4.0 * DEG))
    with NdtMatcher3D(cell_size=1.0) as t, NdtMatcher3D(cell_size=1.0) as s:
        t.set_target(d["tx"], d["ty"], d["tz"])
        s.set_target(d["sx"], d["sy"], d["sz"])
        out = t.search_align_map(s, *window, k=4)
        assert len(out) == 4
        hits = t.search_map(s, *window, k=4)
        assert [h.pose for h in hits] == [h.pose for h, _ in out]
        for h, r in out:
            assert _same(r, t.align_map(s, h.pose)), (h, r)
        multi = t.align_map_multi([s] * len(hits), [h.pose for h in hits])
        assert all(_same(a, r) for a, (_, r) in zip(multi, out))
