"""ndt2d_align_map_multi: up to 64 map-to-map alignments against one target in one launch chain (docs/ALGORITHM.md
section 2.15a).  Every comparison is bitwise against ndt2d_align_map on the same handles from the same pose: there is no
tolerance to choose.

Component counts of the scenes at cell 0.5 (tests/d2d_ref.py agrees): room8 source 116 / first half 90 / first eighth
11, target 151: a 1000-point scan never fills a second 256-component workgroup, so the mixed call of either scene also
takes the OTHER scene's source map (room50: 1065 / 988 / 420, target 1414: 5, 4, 2 and 6 workgroups) and spans two
values of `blocks` on both scenes."""
import ctypes as C
import math

import numpy as np
import pytest

from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import search, synth
from oracle import ndt2d as O

pytestmark = pytest.mark.gpu

SCENES = {"room8": (1, {}), "room50": (2, dict(n_tgt=20_000, n_src=20_000))}
VARIANTS = {
    "converged": dict(),
    "converged_linesearch4": dict(line_search=4),
    "fixed10": dict(fixed_iterations=10),
    "fixed6_relaxed3_linesearch4": dict(fixed_iterations=6, step_scale=3.0, line_search=4),
    "cut8_relaxed3_linesearch4": dict(max_iterations=8, step_scale=3.0, line_search=4),
}
BLOCK, MAX_BLOCKS = 256, 256
DEG = math.pi / 180.0
OFFSET = (1.1, -0.9, 0.35)               # the loop-closure guess of tests/test_gpu_search_map.py
_PAIRS = {}


def _pair(scene):
    if scene not in _PAIRS:
        cfg, kw = SCENES[scene]
        _PAIRS[scene] = synth.make_pair(cfg, **kw)
    return _PAIRS[scene]


def _same(a, b):
    return (a.pose == b.pose and np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g) and a.score == b.score and
            a.iterations == b.iterations and a.n_hit == b.n_hit and a.status == b.status)


def _matcher(x, y, **kw):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    m = NdtMatcher2D(**kw)
    m.set_target(x, y)
    return m


def _handles(d, **kw):
    return _matcher(d["tx"], d["ty"], **kw), _matcher(d["sx"], d["sy"], **kw)


def _blocks(n):
    return min((n + BLOCK - 1) // BLOCK, MAX_BLOCKS)


def _spread(init, m):
    """init, then a deterministic spread around it; every fourth start is metres and a radian off, so that starts end at
    different iterations or with another status."""
    out = []
    for k in range(m):
        dx, dy, dt = 0.12 * ((7 * k) % 5 - 2), 0.09 * ((3 * k) % 7 - 3), 0.03 * ((5 * k) % 9 - 4)
        if k == 0:
            dx = dy = dt = 0.0
        if k % 4 == 3:
            dx, dy, dt = dx + 2.5, dy - 1.5, dt + 0.9 * (1 + k // 16)
        out.append((init[0] + dx, init[1] + dy, init[2] + dt))
    return out


def _check(t, sources, poses, tag=""):
    """one multi call against the single calls from the same poses; returns the multi results"""
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    srcs = [sources] * len(poses) if isinstance(sources, NdtMatcher2D) else list(sources)
    multi = t.align_map_multi(sources, poses)
    assert len(multi) == len(poses)
    for k, (s, p, r) in enumerate(zip(srcs, poses, multi)):
        single = t.align_map(s, p)
        assert _same(r, single), (tag, k, p, r, single)
    return multi


# ---------------------------------------------------------------------------------------------- 1. multi-start identity
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("mode", [O.HESSIAN_GN, O.HESSIAN_NEWTON])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_every_start_equals_its_single_alignment(gpu_lib, scene, mode, variant):
    d = _pair(scene)
    t, s = _handles(d, hessian_mode=mode, **VARIANTS[variant])
    try:
        poses = _spread(d["init"], 64)
        single = [t.align_map(s, p) for p in poses]
        for m in (1, 2, 3, 5, 16, 64):
            multi = t.align_map_multi(s, poses[:m])
            assert len(multi) == m
            for k in range(m):
                assert _same(multi[k], single[k]), (m, k, poses[k], multi[k], single[k])
        its = sorted({r.iterations for r in single})
        sts = sorted({r.status for r in single})
        print(f"{scene} mode {mode} {variant}: iteration counts {its}, statuses {sts}")
        if variant.startswith("converged"):
            assert len(its) >= 2                  # starts finish at different launches: the freezing is exercised
    finally:
        t.close(); s.close()


# ---------------------------------------------------------------------------------------------- 2. mixed sources
@pytest.mark.parametrize("mode", [O.HESSIAN_GN, O.HESSIAN_NEWTON])
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_mixed_sources_in_one_call(gpu_lib, scene, mode):
    d = _pair(scene)
    other = _pair("room50" if scene == "room8" else "room8")
    n = d["sx"].size
    kw = dict(hessian_mode=mode)
    t = _matcher(d["tx"], d["ty"], **kw)
    full = _matcher(d["sx"], d["sy"], **kw)
    half = _matcher(d["sx"][:n // 2], d["sy"][:n // 2], **kw)
    eighth = _matcher(d["sx"][:n // 8], d["sy"][:n // 8], **kw)
    foreign = _matcher(other["sx"], other["sy"], **kw)
    try:
        counts = {name: h.components()[0].size for name, h in
                  (("full", full), ("half", half), ("eighth", eighth), ("target", t), ("other scene", foreign))}
        blocks = {name: _blocks(c) for name, c in counts.items()}
        print(f"{scene}: components {counts}, blocks {blocks}")
        assert min(counts.values()) > 0 and len(set(blocks.values())) >= 2
        init = d["init"]
        near = (init[0] + 0.2, init[1] - 0.1, init[2] + 0.05)
        sources = [full, half, eighth, t, foreign, half, full, half]
        poses = [init, init, init, (0.0, 0.0, 0.0), init, near, near, (init[0] - 0.3, init[1] + 0.2, init[2] - 0.04)]
        _check(t, sources, poses, scene)                      # entry 3: the target against itself, from the identity
        # the narrowest list first and alone in a wide launch, and the widest alone
        _check(t, [eighth, foreign], [init, init], scene)
        _check(t, [foreign if scene == "room8" else full], [init], scene)
    finally:
        for h in (t, full, half, eighth, foreign):
            h.close()


# ---------------------------------------------------------------------------------------------- 3. more than 65 536 components
def test_more_components_than_one_pass_of_the_launch(gpu_lib):
    """blocks capped at 256 workgroups: every lane walks the list in strides of 65 536 components."""
    rng = np.random.default_rng(20240607)
    x = rng.uniform(-80.0, 80.0, 1_000_000).astype(np.float32)
    y = rng.uniform(-80.0, 80.0, 1_000_000).astype(np.float32)
    big = _matcher(x, y, cell_size=0.5, fixed_iterations=6)
    try:
        n_comp = big.components()[0].size
        print(f"{n_comp} components")
        assert n_comp > 65536
        poses = [(0.05, -0.03, 0.002), (-0.04, 0.06, -0.003), (0.02, 0.02, 0.001)]
        multi = _check(big, big, poses)
        assert all(r.iterations == 6 and r.n_hit > 0 for r in multi)
    finally:
        big.close()


# ---------------------------------------------------------------------------------------------- 4. empty participants
def test_empty_participants(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = _pair("room50")
    t, s = _handles(d)
    init = d["init"]
    off = (init[0] + 0.15, init[1] - 0.1, init[2] + 0.02)
    try:
        with NdtMatcher2D() as hollow, NdtMatcher2D(min_points=100_000) as sparse:
            hollow.reserve_target(-27.0, -27.0, 27.0, 27.0)              # a grid that never saw a point
            assert hollow.components()[0].size == 0
            for order in ([s, hollow, s], [hollow, s, s], [s, s, hollow]):
                poses = [init, off, (0.3, -0.2, 0.1)]
                multi = t.align_map_multi(order, poses)
                for h, p, r in zip(order, poses, multi):
                    if h is hollow:
                        assert r.status == O.NDT_TOO_FEW_CELLS and r.pose == p and r.iterations == 0 and r.n_hit == 0
                        assert not r.H.any() and not r.g.any() and r.score == 0.0
                    else:
                        assert _same(r, t.align_map(s, p))
            only = t.align_map_multi([hollow, hollow], [init, off])
            assert [r.status for r in only] == [O.NDT_TOO_FEW_CELLS] * 2 and [r.pose for r in only] == [init, off]
            # a target without a valid cell: every start
            sparse.set_target(d["tx"], d["ty"])
            multi = sparse.align_map_multi([s, t, s], [init, off, init])
            for p, r in zip([init, off, init], multi):
                assert r.status == O.NDT_TOO_FEW_CELLS and r.pose == p and r.iterations == 0 and r.n_hit == 0
            # and the handles go on as before
            _check(t, s, [init, off])
    finally:
        t.close(); s.close()


# ---------------------------------------------------------------------------------------------- 5. launch modes
@pytest.mark.parametrize("opts", [dict(), dict(fixed_iterations=7), dict(hessian_mode=1, line_search=4)],
                         ids=["converged", "fixed7", "newton_linesearch"])
def test_launch_modes_give_the_same_bits(gpu_lib, opts):
    d = _pair("room50")
    n = d["sx"].size
    t, s = _handles(d, **opts)
    half = _matcher(d["sx"][:n // 2], d["sy"][:n // 2], **opts)
    try:
        sources = [s, half, s, half, s]
        poses = _spread(d["init"], 5)
        want = _check(t, sources, poses)

        def again(tag):
            got = t.align_map_multi(sources, poses)
            assert all(_same(a, b) for a, b in zip(got, want)), tag
        t.set_tuning("launch_graphs", 0)
        again("plain launches")
        t.set_tuning("chunk_launches", 3)
        again("plain launches, polled every 3")
        t.set_tuning("launch_graphs", 1)
        for chunk in (2, 8):
            t.set_tuning("chunk_launches", chunk)
            again(f"chunks of {chunk}")
        # the threshold between one chain per start and one chain for all: the same bits on either side
        t.set_tuning("map_multi_from", 65)
        again("one chain per start")
        t.set_tuning("map_multi_from", 1)
        again("one chain for all")
        one = t.align_map_multi(s, poses[:1])
        assert _same(one[0], want[0])
    finally:
        t.close(); s.close(); half.close()


# ---------------------------------------------------------------------------------------------- 6. interleaving
def test_interleaving_with_the_point_to_map_chains(gpu_lib):
    import torch
    d = _pair("room50")
    t, s = _handles(d)
    try:
        sx, sy = torch.from_numpy(d["sx"]).cuda(), torch.from_numpy(d["sy"]).cuda()
        starts = _spread(d["init"], 64)
        p2m = t.align_multi_start(sx, sy, starts)             # all 256 partial rows of all 64 starts are dirty now
        poses = _spread(d["init"], 9)
        first = _check(t, s, poses)
        p2m_again = t.align_multi_start(sx, sy, starts)
        assert all(_same(a, b) for a, b in zip(p2m, p2m_again))
        # directly behind the point-to-map chain, without single calls in between
        second = t.align_map_multi(s, poses)
        third = t.align_map_multi(s, poses)
        assert all(_same(a, b) for a, b in zip(first, second)) and all(_same(a, b) for a, b in zip(first, third))
        assert _same(t.align(sx, sy, d["init"]), p2m[0])
    finally:
        t.close(); s.close()


# ---------------------------------------------------------------------------------------------- 7. the caches
def test_derived_data_follows_the_grid(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    d = _pair("room50")
    box = (-27.0, -27.0, 27.0, 27.0)
    half = d["sx"].size // 2
    poses = _spread(d["init"], 4)
    with NdtMatcher2D() as t, NdtMatcher2D() as s, NdtMatcher2D() as s2, NdtMatcher2D() as fixed_src:
        t.set_target(d["tx"], d["ty"])
        fixed_src.set_target(d["sx"], d["sy"])
        s.reserve_target(*box)
        s.add_target_points(d["sx"][:half], d["sy"][:half])
        sources = [s, fixed_src, s, s]
        before = t.align_map_multi(sources, poses)
        s.add_target_points(d["sx"][half:], d["sy"][half:])
        after = _check(t, sources, poses)                     # fresh single calls on the grown grid
        assert not _same(before[0], after[0]) and _same(before[1], after[1])
        s2.reserve_target(*box)
        s2.add_target_points(d["sx"], d["sy"])
        fresh = t.align_map_multi([s2, fixed_src, s2, s2], poses)
        assert all(_same(a, b) for a, b in zip(after, fresh))


# ---------------------------------------------------------------------------------------------- 8. the error table
def test_error_table_leaves_the_handles_intact(gpu_lib):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    lib = gpu_lib
    d = _pair("room8")
    init = d["init"]
    with NdtMatcher2D() as t, NdtMatcher2D() as s, NdtMatcher2D() as empty, NdtMatcher2D(overlap_grids=4) as four:
        t.set_target(d["tx"], d["ty"])
        s.set_target(d["sx"], d["sy"])
        four.set_target(d["sx"], d["sy"])
        good_poses = _spread(init, 3)
        want = _check(t, s, good_poses)

        def intact():
            got = t.align_map_multi(s, good_poses)
            assert all(_same(a, b) for a, b in zip(got, want))
            assert _same(s.align_map_multi(t, [(0.0, 0.0, 0.0)])[0], s.align_map(t, (0.0, 0.0, 0.0)))

        res = (L.Result2D * 64)()
        rp = C.cast(res, C.c_void_p)
        poses = (C.c_double * 9)(*[v for p in good_poses for v in p])

        def call(target, sources, p=poses, m=3, r=rp):
            hs = None if sources is None else (C.c_void_p * 64)(*[h._h.value if h is not None else None for h in sources])
            return lib.ndt2d_align_map_multi(target._h if target is not None else None, hs, p, m, r)

        # null pointers, a null entry
        assert call(None, [s, s, s]) == L.NDT_ERR_INVALID_ARG
        assert call(t, None) == L.NDT_ERR_INVALID_ARG
        assert call(t, [s, s, s], p=None) == L.NDT_ERR_INVALID_ARG
        assert call(t, [s, s, s], r=None) == L.NDT_ERR_INVALID_ARG
        assert call(t, [s, None, s]) == L.NDT_ERR_INVALID_ARG
        intact()
        # m out of range
        big = (C.c_double * (3 * 65))()
        for m in (0, 65, -1):
            assert call(t, [s] * 64, p=big, m=m) == L.NDT_ERR_INVALID_ARG
        intact()
        # a non-finite pose, in any start
        for bad in (float("nan"), float("inf"), -float("inf")):
            for j in range(9):
                p = (C.c_double * 9)(*poses)
                p[j] = bad
                assert call(t, [s, s, s], p=p) == L.NDT_ERR_INVALID_ARG
        intact()
        # overlapping grids on the target or on any source
        for target, sources in ((four, [s, s, s]), (t, [s, s, four]), (t, [four, s, s])):
            assert call(target, sources) == L.NDT_ERR_INVALID_ARG
            assert b"overlapping grids" in lib.ndt_last_error()
        intact()
        # a handle without a grid
        for target, sources in ((empty, [s, s, s]), (t, [s, empty, s]), (t, [empty, empty, empty])):
            assert call(target, sources) == L.NDT_ERR_NO_TARGET
        intact()
        if lib.ndt_device_count() >= 2:
            import torch
            with NdtMatcher2D(device=1) as far:
                far.set_target(d["sx"], d["sy"])
                assert call(t, [s, far, s]) == L.NDT_ERR_INVALID_ARG
                assert call(far, [s, s, s]) == L.NDT_ERR_INVALID_ARG
            torch.cuda.set_device(0)
            intact()
        else:
            print("one device: the different-devices row cannot be built here")
        # the Python wrapper: one pose per source
        with pytest.raises(ValueError):
            t.align_map_multi([s, s], good_poses)
        with pytest.raises(L.NdtError):
            t.align_map_multi(s, [init] * 65)
        intact()


# ---------------------------------------------------------------------------------------------- 9. search_align_map
def test_search_align_map_refines_through_the_multi_call(gpu_lib):
    d = _pair("room50")
    guess = tuple(a + b for a, b in zip(d["pose"], OFFSET))
    window = search.Window(guess, (2.0, 2.0, math.pi), (0.25, 0.25, 4.0 * DEG))
    t, s = _handles(d)
    try:
        out = t.search_align_map(s, *window, k=8)
        assert len(out) == 8
        for h, r in out:
            assert _same(r, t.align_map(s, h.pose)), (h, r)
        multi = t.align_map_multi([s] * len(out), [h.pose for h, _ in out])
        assert all(_same(a, r) for a, (_, r) in zip(multi, out))
    finally:
        t.close(); s.close()
