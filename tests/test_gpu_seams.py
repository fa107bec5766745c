"""Every kernel family that looks a point up in the grid, held hit for hit - integer equality, no slack, no excused
points - to the exact restatement of its own image and key rule (tests/seam_ref.py) on the seam catalogue
(tests/seam_cases.py): every source point has its image on a cell seam or one ulp below it, on the ring, at the grid's
edge, far outside, or is not finite; validity is a checkerboard, so one misplaced point flips a hit.

Families that return a score only (score_poses, the search volumes) are held to the float64 score from the reference keys
within the tolerance of their own tests (1e-4 |ref| + 1e-3) on sources of 16 one-seam points, where the smallest single
term is more than 100 times that tolerance (asserted on the CPU in tests/test_seam_ref.py).

The target side: the min_points-exact targets (a valid cell holds exactly min_points points, one of them on the cell's own
seam or one ulp outside it) through every build, per-cell counts equal to the reference's; the batch kernels' own build
through a one-point probe at every cell's centre (the valid bit).

The map-to-map families (evaluate_map, align_map, score_map_poses) look a component's mean up: the source map's means
are read back (components()), and translations are searched that put a mean exactly on a seam of the target, or one ulp
below it; the hit count is that of the chain image of every mean.  (search_map returns scores only and shares
score_map_poses' lookup to the bit, which tests/test_gpu_search_map*.py hold; it is not repeated here.)"""
import functools

import numpy as np
import pytest

import seam_cases as K
import seam_ref as S

pytestmark = pytest.mark.gpu

SIZES = (63, 64, 65, 256, 1000, 4097)
NDT_OK, NDT_NOT_CONVERGED, NDT_DEGENERATE_HESSIAN, NDT_TOO_FEW_HITS = 0, 1, 2, 3
ONE = dict(fixed_iterations=1, min_hits=1)


def _api(dim):
    from gtsam_ndt_amd import matcher as M
    return (M.NdtMatcher2D, M.NdtBatch2D) if dim == 2 else (M.NdtMatcher3D, M.NdtBatch3D)


def _targets(dim):
    """[(target, [(pose name, pose, source)])] over the catalogue"""
    out = {}
    for c, base, pn in K.entries(dim):
        out.setdefault((c, base), []).append((pn, K.POSES[dim][pn], K.source(dim, c, base, pn)))
    return [(K.target(dim, c, base), v) for (c, base), v in out.items()]


@functools.lru_cache(maxsize=None)
def _packed(dim, c, base, pn, n, stretch=0):
    """(coords, expected hits per family recipe) of the entry's source packed to n points"""
    t, src, pose = K.target(dim, c, base, False, stretch), K.source(dim, c, base, pn, stretch), K.POSES[dim][pn]
    coords, _ = K.packed(src, n)
    want = {"chain": K.n_hit(t, coords, pose)}
    if dim == 3:
        want["batch3"] = K.n_hit(t, coords, pose, family="batch3")
        want["nb7"] = K.n_hit(t, coords, pose, neighbourhood=7)
    return coords, want


def _cuda(coords):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in coords)


def _what(t, pn, more=""):
    return f"{t.name} @ {pn} {more}"


# ---------------------------------------------------------------------------------------------- evaluate
@pytest.mark.parametrize("dim", [2, 3])
def test_evaluate_counts_every_seam_point(gpu_lib, dim):
    Matcher, _ = _api(dim)
    checked = 0
    for t, poses in _targets(dim):
        with Matcher(**t.kw) as m, Matcher(**t.kw, **ONE) as one:
            m.set_target(*t.coords)
            one.set_target(*t.coords)
            for pn, pose, src in poses:
                hits, _ = K.point_hits(t, src.coords, pose)
                H, g, score, n_hit = m.evaluate(*src.coords, pose)
                assert n_hit == hits.sum(), _what(t, pn, f"whole source: {n_hit} hits, reference {hits.sum()}")
                # non-finite points change nothing
                fin = S.finite_points(*src.coords)
                H2, g2, score2, n2 = m.evaluate(*[a[fin] for a in src.coords], pose)
                assert n2 == n_hit and score2 == score and np.array_equal(H2, H) and np.array_equal(g2, g), _what(t, pn)
                for n in SIZES:
                    coords, want = _packed(dim, t.c, t.base, pn, n)
                    assert m.evaluate(*coords, pose)[3] == want["chain"], _what(t, pn, f"{n} points")
                # one-point sources: the hit is the valid bit; a miss is exact zeros and NDT_TOO_FEW_HITS
                pick = np.concatenate([np.flatnonzero(hits > 0)[:3], np.flatnonzero(hits == 0)[:3], [len(hits) - 1]])
                for j in pick:
                    pt = [a[j:j + 1] for a in src.coords]
                    r = one.align(*pt, pose)
                    assert r.n_hit == hits[j], _what(t, pn, f"point {j} {[float(v[0]) for v in pt]}")
                    if hits[j] == 0:
                        assert r.status == NDT_TOO_FEW_HITS and r.score == 0.0 and not r.H.any() and not r.g.any(), _what(t, pn)
                    else:
                        assert r.status in (NDT_OK, NDT_NOT_CONVERGED, NDT_DEGENERATE_HESSIAN), _what(t, pn, r.status)
                checked += 1
    assert checked == len(K.entries(dim))


# ---------------------------------------------------------------------------------------------- align, one evaluation
PATHS_2D = {
    "k_align_small": {},
    "k_iterate_first_graph": {"short_scan_kernel": 0},
    "k_iterate_plain_launches": {"short_scan_kernel": 0, "launch_graphs": 0},
    "k_begin": {"short_scan_kernel": 0, "fused_begin": 0},
    "k_begin_plain_launches": {"short_scan_kernel": 0, "fused_begin": 0, "launch_graphs": 0},
    "wide_1024": {"short_scan_kernel": 0, "wide_threshold": 60},
}


@pytest.mark.parametrize("path", list(PATHS_2D))
def test_align_2d_first_evaluation(gpu_lib, path):
    """align(fixed_iterations = 1): n_hit is that of the evaluation at the initial pose, through every launch path."""
    Matcher, _ = _api(2)
    for t, poses in _targets(2):
        with Matcher(tuning=PATHS_2D[path], **t.kw, **ONE) as m:
            m.set_target(*t.coords)
            for pn, pose, _ in poses:
                for n in SIZES:
                    coords, want = _packed(2, t.c, t.base, pn, n)
                    r = m.align(*coords, pose)
                    assert r.n_hit == want["chain"], _what(t, pn, f"{path}, {n} points: {r.n_hit} hits, reference {want['chain']}")
                    assert r.iterations <= 1


@pytest.mark.parametrize("neighbourhood,fused", [(1, 1), (1, 0), (7, 1), (7, 0)])
def test_align_3d_first_evaluation(gpu_lib, neighbourhood, fused):
    """The same in 3D, own voxel and with the six face neighbours (taken by index at a first or last voxel: the
    catalogue's sources sit on the grid's outer seams too)."""
    Matcher, _ = _api(3)
    key = "chain" if neighbourhood == 1 else "nb7"
    for t, poses in _targets(3):
        with Matcher(tuning={"fused_begin": fused}, neighbourhood=neighbourhood, **t.kw, **ONE) as m:
            m.set_target(*t.coords)
            for pn, pose, src in poses:
                for n in SIZES:
                    coords, want = _packed(3, t.c, t.base, pn, n)
                    r = m.align(*coords, pose)
                    assert r.n_hit == want[key], _what(t, pn, f"neighbourhood {neighbourhood}, {n} points: {r.n_hit} / {want[key]}")
                if neighbourhood == 7:
                    assert m.evaluate(*src.coords, pose)[3] == K.n_hit(t, src.coords, pose, neighbourhood=7), _what(t, pn)


@pytest.mark.parametrize("dim,split_from", [(2, 1), (2, 1000), (3, None)])
def test_multi_start_and_multi_scan(gpu_lib, dim, split_from):
    """k_iterate_multi / k_multi_body: several starts of one scan (each of the target's poses), and several scans, fused
    (split_from above the count) and split."""
    Matcher, _ = _api(dim)
    for t, poses in _targets(dim):
        tuning = {"split_from": split_from} if dim == 2 else {}
        with Matcher(tuning=tuning, **t.kw, **ONE) as m:
            m.set_target(*t.coords)
            pn0, pose0, src0 = poses[0]
            coords, _ = K.packed(src0, 1000)
            starts = [p for _, p, _ in poses]
            got = [r.n_hit for r in m.align_multi_start(*_cuda(coords), starts)]
            assert got == [K.n_hit(t, coords, p) for p in starts], _what(t, pn0, "multi-start")
            scans, inits, want = [], [], []
            for pn, pose, _ in poses:
                for n in (65, 1000, 4097):
                    cc, w = _packed(dim, t.c, t.base, pn, n)
                    scans.append(_cuda(cc)); inits.append(pose); want.append(w["chain"])
            got = [r.n_hit for r in m.align_multi_scan(scans, inits)]
            assert got == want, _what(t, "all poses", "multi-scan")


# ---------------------------------------------------------------------------------------------- batch kernels
def _batch_pairs(dim, t, poses, sizes, family):
    sources, inits, want, names = [], [], [], []
    for pn, pose, src in poses:
        for n in sizes:
            coords, w = _packed(dim, t.c, t.base, pn, n, t.stretch)
            sources.append(coords); inits.append(pose); want.append(w[family]); names.append(f"{pn} {n} points")
    return sources, inits, want, names


@pytest.mark.parametrize("variant", ["small", "1024", "global"])
def test_batch_2d(gpu_lib, variant):
    """lookup_point_lds of the three k_batch variants; the global-table grid on targets stretched past 143 x 143 cells."""
    _, Batch = _api(2)
    how = {"small": dict(small_variant=True), "1024": dict(small_variant=False), "global": dict(global_workgroups=8)}[variant]
    for c, base in K.TARGETS_2D:
        stretch = 150 if variant == "global" else 0
        t = K.target(2, c, base, False, stretch)
        if stretch:
            assert t.ext[0] * t.ext[1] > 143 * 143
        poses = [(pn, K.POSES[2][pn], K.source(2, c, base, pn, stretch)) for cc, bb, pn in K.entries(2) if (cc, bb) == (c, base)]
        sources, inits, want, names = _batch_pairs(2, t, poses, (63, 65, 1000, 4097), "chain")
        with Batch(**how, **t.kw, **ONE) as b:
            res = b.align([t.coords] * len(sources), sources, inits)
            large = b.last_large_count
        assert large == (0 if variant == "small" else len(sources)), (variant, large)
        got = [r.n_hit for r in res]
        assert got == want, (t.name, variant, [(n_, g_, w_) for n_, g_, w_ in zip(names, got, want) if g_ != w_])


def test_batch_2d_four_overlapping_grids(gpu_lib):
    """overlap_grids = 4: a point counts once per grid whose cell is valid (ALGORITHM 2.7); the batch, the single-pair
    handle with the same option and the reference agree."""
    Matcher, Batch = _api(2)
    for t, poses in _targets(2)[::2]:
        sources, inits, want = [], [], []
        for pn, pose, src in poses:
            coords, _ = K.packed(src, 1000)
            sources.append(coords); inits.append(pose); want.append(K.n_hit(t, coords, pose, overlap=4))
        with Matcher(overlap_grids=4, **t.kw) as m:
            m.set_target(*t.coords)
            single = [m.evaluate(*cc, p)[3] for cc, p in zip(sources, inits)]
        with Batch(overlap_grids=4, **t.kw, **ONE) as b:
            got = [r.n_hit for r in b.align([t.coords] * len(sources), sources, inits)]
        assert single == want, (t.name, single, want)
        assert got == want, (t.name, got, want)


@pytest.mark.parametrize("variant", ["onchip", "global"])
def test_batch_3d(gpu_lib, variant):
    """k_batch3 forms y = R p by the fmaf chain and then p' = y + t: its own recipe (seam_ref.image3d_batch), one rounding
    more than every other 3D kernel's.  Global tables: targets stretched to 27^3 voxels."""
    _, Batch = _api(3)
    how = dict(global_workgroups=8) if variant == "global" else {}
    differs = 0
    for c, base in K.TARGETS_3D:
        stretch = 27 if variant == "global" else 0
        t = K.target(3, c, base, False, stretch)
        if stretch:
            assert int(np.prod(t.ext)) > 17424
        poses = [(pn, K.POSES[3][pn], K.source(3, c, base, pn, stretch)) for cc, bb, pn in K.entries(3) if (cc, bb) == (c, base)]
        sources, inits, want, names = _batch_pairs(3, t, poses, (63, 65, 1000, 4097), "batch3")
        with Batch(**how, **t.kw, **ONE) as b:
            got = [r.n_hit for r in b.align([t.coords] * len(sources), sources, inits)]
        assert got == want, (t.name, variant, [(n_, g_, w_) for n_, g_, w_ in zip(names, got, want) if g_ != w_])
        differs += sum(K.n_hit(t, cc, p, family="chain") != w for cc, p, w in zip(sources, inits, want))
    assert differs > 0          # the catalogue does tell the two recipes apart


# ---------------------------------------------------------------------------------------------- pose lists
@pytest.mark.parametrize("dim,team", [(2, 64), (2, 256), (3, 64), (3, 256)])
def test_score_particles_hit_counts(gpu_lib, dim, team):
    Matcher, _ = _api(dim)
    for t, poses in _targets(dim):
        with Matcher(tuning={"particle_team": team}, **t.kw) as m:
            m.set_target(*t.coords)
            plist = np.array([p for _, p, _ in poses], np.float64)
            for pn, pose, src in poses:
                coords, _ = K.packed(src, 1000)
                _, cnt = m.score_particles(*coords, plist, with_hits=True)
                want = [K.n_hit(t, coords, p) for p in plist]
                assert [int(v) for v in cnt] == want, _what(t, pn, f"team {team}")


@pytest.mark.parametrize("dim", [2, 3])
def test_score_poses_and_search_volume(gpu_lib, dim):
    """Score-only families: the float64 score from the reference keys; one wrong cell moves it by a whole term, at least
    100 tolerances.  Measured on an MI355X: the worst error is 0.0012 of the tolerance in 2D, 0.0004 in 3D."""
    Matcher, _ = _api(dim)
    worst = 0.0
    for t, poses in _targets(dim):
        with Matcher(**t.kw) as m:
            m.set_target(*t.coords)
            plist = np.array([p for _, p, _ in poses], np.float64)
            for pn, pose, src in poses:
                for coords, _, _ in K.score_packs(t, src, pose, n_packs=3):
                    want = np.array([K.score_terms(t, coords, p).sum() for p in plist])
                    got = np.asarray(m.score_poses(*coords, plist), np.float64)
                    tol = np.array([K.score_tolerance(w) for w in want])
                    assert np.all(np.abs(got - want) <= tol), _what(t, pn, f"score_poses {got} reference {want}")
                    worst = max(worst, float(np.max(np.abs(got - want) / tol)))
                    # the search volume on a 3 x 3 lattice round the pose: its centre is the pose itself
                    # (3D: over x, y and yaw, the other three pinned to the pose's; the z seams go through layer_key3)
                    vol = m.search_scores(*coords, pose, (0.25, 0.25, 0.0), (0.25, 0.25, 0.1))
                    assert tuple(vol.shape) == (1, 3, 3)
                    centre = float(vol[0, 1, 1])
                    w = K.score_terms(t, coords, pose).sum()
                    assert abs(centre - w) <= K.score_tolerance(w), _what(t, pn, f"search volume {centre} reference {w}")
    print(f"dim {dim}: worst score error / tolerance {worst:.3g}")


@pytest.mark.parametrize("dim", [2, 3])
def test_fit_points_class_of_every_point(gpu_lib, dim):
    """fit_points / select_points: invalid, miss or hit, exact at every point of every pose (no point is excused)."""
    Matcher, _ = _api(dim)
    for t, poses in _targets(dim):
        with Matcher(**t.kw) as m:
            m.set_target(*t.coords)
            for pn, pose, src in poses:
                hits, _ = K.point_hits(t, src.coords, pose)
                fin = S.finite_points(*src.coords)
                want = np.where(fin, np.where(hits > 0, 2, 1), 0)
                fit = m.fit_points(*src.coords, pose, 1e30)
                got = np.minimum(np.asarray(fit.cls, np.int64), 2)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, _what(t, pn, f"{bad.size} points differ, first {bad[:5]}: {got[bad[:5]]} / {want[bad[:5]]}")
                assert (fit.n_invalid, fit.n_miss, fit.n_misfit + fit.n_fit) == (int((want == 0).sum()), int((want == 1).sum()), int((want == 2).sum()))
                kept, index, _ = m.select_points(*src.coords, pose, 1e30, keep=("fit", "misfit"))
                assert np.array_equal(np.asarray(index), np.flatnonzero(want == 2)), _what(t, pn, "select_points")


def test_fit_points_four_overlapping_grids(gpu_lib):
    Matcher, _ = _api(2)
    for t, poses in _targets(2)[1::3]:
        with Matcher(overlap_grids=4, **t.kw) as m:
            m.set_target(*t.coords)
            for pn, pose, src in poses:
                hits, _ = K.point_hits(t, src.coords, pose, overlap=4)
                fin = S.finite_points(*src.coords)
                want = np.where(fin, np.where(hits > 0, 2, 1), 0)
                got = np.minimum(np.asarray(m.fit_points(*src.coords, pose, 1e30).cls, np.int64), 2)
                assert np.array_equal(got, want), _what(t, pn, f"{int((got != want).sum())} points differ")
                assert m.evaluate(*src.coords, pose)[3] == hits.sum(), _what(t, pn)


# ---------------------------------------------------------------------------------------------- the target side
def _reference_counts(t):
    return np.asarray(t.grid.count, np.int64)


BUILDS_2D = {"binned": {}, "atomic": {"binned_build": 0}, "two_round_trips": {"single_sync_build": 0},
             "atomic_two_round_trips": {"binned_build": 0, "single_sync_build": 0}}


@pytest.mark.parametrize("build", list(BUILDS_2D))
def test_target_build_2d_counts(gpu_lib, build):
    """set_target on the min_points-exact targets: per-cell counts, hence validity, equal to the reference's; the second
    build on the same handle goes through the single-sync path (or not); then add and remove at a float32 translation."""
    Matcher, _ = _api(2)
    for c, base in K.TARGETS_2D:
        t, other = K.target(2, c, base, True), K.target(2, c, base, False)
        with Matcher(tuning=BUILDS_2D[build], **t.kw) as m:
            m.set_target(*other.coords)                       # a grid is cached: the next build may decide its geometry on the device
            info = m.set_target(*t.coords)
            assert (info.width, info.height, info.ox, info.oy) == (t.grid.W, t.grid.H, t.grid.ox, t.grid.oy), t.name
            count, _, icov = m.grid()
            assert np.array_equal(count.astype(np.int64), _reference_counts(t)), (t.name, build)
            assert np.array_equal(icov[:, 0] != 0, t.grid.valid), (t.name, build)
            assert info.n_valid == t.grid.n_valid
            # add the same cloud again through a pose, then remove it.  A float32 translation without rotation: the image
            # (k_transform_points: (cs x - sn y) + tx, separate roundings) is one float32 add per axis, as in the chain
            shift = (0.25, -0.5, 0.0)
            sx, sy = (t.coords[0] - np.float32(shift[0])).astype(np.float32), (t.coords[1] - np.float32(shift[1])).astype(np.float32)
            ix, iy = S.image2d(sx, sy, shift)
            key, inside = S.o2.cell_keys32(ix, iy, *t.geom, interior=True)
            added = np.bincount(key[inside], minlength=len(count)).astype(np.int64)
            n_out = m.add_target_points(*_cuda((sx, sy)), pose=shift)
            assert n_out == int((~inside).sum()), (t.name, build)
            assert np.array_equal(m.grid()[0].astype(np.int64), _reference_counts(t) + added), (t.name, build, "add")
            m.remove_target_points(*_cuda((sx, sy)), pose=shift)
            assert np.array_equal(m.grid()[0].astype(np.int64), _reference_counts(t)), (t.name, build, "remove")


@pytest.mark.parametrize("sync", [1, 0])
def test_target_build_3d_counts(gpu_lib, sync):
    Matcher, _ = _api(3)
    for c, base in K.TARGETS_3D:
        t, other = K.target(3, c, base, True), K.target(3, c, base, False)
        with Matcher(tuning={"single_sync_build": sync}, **t.kw) as m:
            m.set_target(*other.coords)
            info = m.set_target(*t.coords)
            assert (info.width, info.height, info.depth) == tuple(t.grid.dims), t.name
            count, _, icov = m.grid()
            assert np.array_equal(count.astype(np.int64), _reference_counts(t)), (t.name, sync)
            assert np.array_equal(icov[:, 0] != 0, t.grid.valid), (t.name, sync)
            # the same cloud once more through a float32 translation (k_transform_points3: ((r0 x + r1 y) + r2 z) + t is one
            # float32 add per axis without rotation, as the chain), then out again.  3D bins every voxel of the grid.
            shift = (0.25, -0.5, 0.125, 0.0, 0.0, 0.0)
            moved = tuple((t.coords[a] - np.float32(shift[a])).astype(np.float32) for a in range(3))
            key, inside, _ = S.keys3d(*S.image3d(*moved, shift), t.geom)
            added = np.bincount(key[inside], minlength=len(count)).astype(np.int64)
            assert m.add_target_points(*_cuda(moved), pose=shift) == int((~inside).sum()), (t.name, sync)
            assert np.array_equal(m.grid()[0].astype(np.int64), _reference_counts(t) + added), (t.name, sync, "add")
            m.remove_target_points(*_cuda(moved), pose=shift)
            assert np.array_equal(m.grid()[0].astype(np.int64), _reference_counts(t)), (t.name, sync, "remove")


def _centre_probes(t):
    """One probe per cell at the cell's centre (float32; a centre is at least a quarter cell from every seam)."""
    mids = [(0.5 * (t.seams[a][:-1].astype(np.float64) + t.seams[a][1:].astype(np.float64))).astype(np.float32)[:K.SIDE[t.dim] + 2]
            for a in range(t.dim)]
    grid = np.array(np.meshgrid(*mids, indexing="ij")).reshape(t.dim, -1).T
    return [tuple(np.ascontiguousarray(p[a:a + 1]) for a in range(t.dim)) for p in grid]


@pytest.mark.parametrize("variant", ["2d-small", "2d-1024", "2d-global", "3d-onchip", "3d-global"])
def test_batch_build_valid_bits(gpu_lib, variant):
    """The build inside k_batch / k_batch3 has no read-back: the valid bit of every checkerboard cell of the
    min_points-exact targets, read by a one-point probe at the cell's centre at the identity."""
    dim = int(variant[0])
    _, Batch = _api(dim)
    how = {"2d-small": dict(small_variant=True), "2d-1024": dict(small_variant=False), "2d-global": dict(global_workgroups=8),
           "3d-onchip": {}, "3d-global": dict(global_workgroups=8)}[variant]
    stretch = {"2d-global": 150, "3d-global": 27}.get(variant, 0)
    zero = (0.0,) * (3 if dim == 2 else 6)
    for c, base in (K.TARGETS_2D if dim == 2 else K.TARGETS_3D)[::2]:
        t = K.target(dim, c, base, True, stretch)
        probes = _centre_probes(t)
        want = [K.n_hit(t, p, zero, family="batch3" if dim == 3 else "chain") for p in probes]
        assert 0 < sum(want) < len(want)
        with Batch(**how, **t.kw, **ONE) as b:
            res = b.align([t.coords] * len(probes), probes, [zero] * len(probes))
        got = [r.n_hit for r in res]
        assert got == want, (t.name, variant, int(np.sum(np.array(got) != np.array(want))))
        assert all(r.status == NDT_TOO_FEW_HITS and r.score == 0.0 for r, w in zip(res, want) if w == 0), (t.name, variant)


def test_ring_voxels_and_neighbours_by_index(gpu_lib):
    """A reserved 3D grid whose first and last voxel of every x row hold points (3D bins the ring): a face neighbour is
    taken by index, so the +x neighbour of a row's last voxel does not exist - by key arithmetic it would be the first
    voxel of the next row, which is valid here (tests/test_seam_ref.py: the mutant is told apart on this case)."""
    Matcher, _ = _api(3)
    t, (lo, hi), src = K.ring_case()
    zero = (0.0,) * 6
    for nb in (1, 7):
        with Matcher(neighbourhood=nb, **t.kw, **ONE) as m:
            info = m.reserve_target(lo, hi)
            assert (info.width, info.height, info.depth) == tuple(t.grid.dims)
            assert (info.ox, info.oy, info.oz) == tuple(np.float32(v) for v in t.grid.o)
            assert m.add_target_points(*t.coords) == 0
            count, _, icov = m.grid()
            assert np.array_equal(count.astype(np.int64), t.grid.count) and np.array_equal(icov[:, 0] != 0, t.grid.valid)
            want = K.n_hit(t, src, zero, neighbourhood=nb)
            assert m.evaluate(*src, zero)[3] == want
            assert m.align(*src, zero).n_hit == want
            assert want != K.n_hit(t, src, zero, neighbourhood=nb, neighbours_by_key=True) or nb == 1


def _seam_translations(t, mean, n_poses=24):
    """Poses without rotation whose float32 translation puts one component mean exactly on a seam of the target on one
    axis (or one ulp below it): t = seam - mean, then a few float32 neighbours of it are tried on the exact image."""
    dim = t.dim
    rng = np.random.default_rng([29, len(mean)])
    poses = []
    for _ in range(400):
        if len(poses) == n_poses:
            break
        i, a = int(rng.integers(len(mean))), int(rng.integers(dim))
        k = int(rng.integers(1, t.ext[a]))
        goal = t.seams[a][k] if rng.integers(2) else S.below(t.seams[a][k])
        t0 = np.float32(float(goal) - float(mean[i, a]))
        for step in (0, 1, -1, 2, -2):
            ta = t0 + np.float32(step) * np.spacing(np.abs(t0))
            if np.float32(mean[i, a] + np.float32(ta)) == goal:
                tr = [0.0] * dim
                tr[a] = float(ta)
                tr[(a + 1) % dim] = 0.25 * (len(poses) % 3 - 1)
                poses.append(tuple(tr) + (0.0,) * (1 if dim == 2 else 3))
                break
    assert len(poses) >= n_poses // 2
    return poses


@pytest.mark.parametrize("dim", [2, 3])
def test_map_to_map_families_look_the_component_means_up_exactly(gpu_lib, dim):
    Matcher, _ = _api(dim)
    rotated = K.POSES[dim]["generic_a"], K.POSES[dim]["quarter" if dim == 2 else "yaw_quarter"], K.POSES[dim]["beyond_pi"]
    for c, base in (K.TARGETS_2D if dim == 2 else K.TARGETS_3D)[::3]:
        t = K.target(dim, c, base)
        with Matcher(**t.kw, **ONE) as target, Matcher(**t.kw) as source:
            target.set_target(*t.coords)
            source.set_target(*t.coords)
            _, mean, _ = source.components()
            assert len(mean) == t.grid.n_valid
            cols = tuple(np.ascontiguousarray(mean[:, a]) for a in range(dim))
            poses = _seam_translations(t, mean) + list(rotated)
            want = [K.n_hit(t, cols, p) for p in poses]
            on_seam = 0
            for p in poses[:len(poses) - len(rotated)]:
                img = K.image(dim, cols, p)
                on_seam += int(sum(np.isin(img[a], t.seams[a]).sum() + np.isin(img[a], [S.below(v) for v in t.seams[a]]).sum()
                                   for a in range(dim)) > 0)
            assert on_seam == len(poses) - len(rotated)
            _, cnt = target.score_map_poses(source, np.array(poses, np.float64), with_hits=True)
            assert [int(v) for v in cnt] == want, (t.name, "score_map_poses")
            for p, w in zip(poses, want):
                assert target.evaluate_map(source, p)[3] == w, (t.name, p, "evaluate_map")
                assert target.align_map(source, p).n_hit == w, (t.name, p, "align_map")
            assert len(set(want)) > 2
