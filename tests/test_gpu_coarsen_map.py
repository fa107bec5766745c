"""ndt2d_coarsen_map on the device: a submap at 2x or 4x the cell size from a submap's exact sums (docs/ALGORITHM.md
section 2.17).  The definition is integer arithmetic, so the device must give the bytes of tests/map_coarsen_ref.py; what
it derives must agree with a ndt2d_set_target at the coarse cell from the same points (geometry and counts equal, sums
within map_coarsen_ref.sum_bounds), and the coarse handle must be what a handle is after ndt2d_load_map.

Scenes (coarsen_cases.lattice_cloud, coordinates on a 2^-11 lattice so that both paths bin every point alike - asserted):
"tiny" 13 x 11 fine cells of 0.5 m, a few hundred points, plus one fine cell of five identical points alone in its parent
(off the 2^-11 lattice, so that the roundings and the degenerate-cell clamp act - asserted); "wide" 301 x 201 cells, 20 000
points, many workgroups.  Both: origin cells negative and no multiple of f, interior extents no multiple of f, interior
cells next to the ring occupied on all four sides."""
import numpy as np
import pytest

import coarsen_cases as K
import map_coarsen_ref as R

pytestmark = pytest.mark.gpu

C0 = 0.5
SCENES = {"tiny": ((-7, -5), (13, 11), 300), "wide": ((-151, -101), (301, 201), 20000)}
_cache = {}


def _points(scene):
    if scene not in _cache:
        k0, ext, n = SCENES[scene]
        hole = ((0.0, 0.0), (2.0, 2.0)) if scene == "tiny" else None       # one parent at f = 4, four at f = 2
        pts = K.lattice_cloud(17, k0, ext, C0, n, hole)
        if scene == "tiny":
            p = np.array([1.8 + 2.0 ** -23, 1.8 + 5 * 2.0 ** -23])      # towards the upper corner of its parent at both factors
            pts = np.vstack([pts, np.repeat(p[None, :], 5, axis=0)]).astype(np.float32)
        _cache[scene] = pts
    return _cache[scene]


def _scan(pts, n=400):
    """A small scan of the scene: some of its points, a few centimetres off."""
    rng = np.random.default_rng(2)
    q = pts[rng.choice(len(pts), size=min(n, len(pts)), replace=False)].astype(np.float64)
    cs, sn = np.cos(0.004), np.sin(0.004)
    x = cs * q[:, 0] - sn * q[:, 1] + 0.03
    y = sn * q[:, 0] + cs * q[:, 1] - 0.02
    return x.astype(np.float32), y.astype(np.float32)


@pytest.mark.parametrize("f", [2, 4])
@pytest.mark.parametrize("scene", ["tiny", "wide"])
def test_coarsened_submap(gpu_lib, scene, f):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    pts = _points(scene)
    K.assert_lattice_is_awkward(SCENES[scene][0], SCENES[scene][1], f)
    assert K.bins_alike(pts, C0, f)
    x, y = pts[:, 0].copy(), pts[:, 1].copy()
    sx, sy = _scan(pts)
    coarse = dict(cell_size=f * C0, eig_ratio=0.03)
    with NdtMatcher2D(cell_size=C0) as src, NdtMatcher2D(**coarse) as dst, NdtMatcher2D(**coarse) as direct, \
            NdtMatcher2D(**coarse) as loaded, NdtMatcher2D(**coarse) as other:
        src.set_target(x, y)
        fine_blob = src.save_map()
        if scene == "tiny":
            assert K.clamp_was_needed(fine_blob, f)
        dst.set_target(sx, sy)                                   # stale records of another map
        n_valid = src.coarsen_into(dst)
        blob = dst.save_map()
        # the definition, byte for byte, header included
        assert np.array_equal(blob, R.map_coarsen_ref(fine_blob, f))
        # against a build from the same points at the coarse cell
        direct.set_target(x, y)
        worst = R.check_against_direct(blob, direct.save_map(), f)
        print(f"{scene} f={f}: largest |coarsened - direct| first sums {worst[0]}, second sums {worst[1]}")
        idst, idir = dst.grid_info(), direct.grid_info()
        assert (idst.ox, idst.oy, idst.width, idst.height, idst.n_points) == (idir.ox, idir.oy, idir.width, idir.height, idir.n_points)
        assert n_valid == idst.n_valid and n_valid > 0
        # dst is what a handle is after load_map
        loaded.load_map(blob)
        K.same_grid(dst, loaded)
        K.same_result(dst.align(sx, sy, (0.0, 0.0, 0.0)), loaded.align(sx, sy, (0.0, 0.0, 0.0)))
        other.set_target(sx, sy)
        K.same_result(dst.align_map(other, (0.0, 0.0, 0.0)), loaded.align_map(other, (0.0, 0.0, 0.0)))
        K.same_result(other.align_map(dst, (0.0, 0.0, 0.0)), other.align_map(loaded, (0.0, 0.0, 0.0)))
        # it takes points, and gives them back
        out_add = dst.add_target_points(sx, sy)
        assert not np.array_equal(dst.save_map(), blob)
        assert dst.remove_target_points(sx, sy) == out_add
        assert np.array_equal(dst.save_map(), blob)
        # src is unchanged
        assert np.array_equal(src.save_map(), fine_blob)


def test_coarsen_twice_equals_coarsen_by_four_in_geometry(gpu_lib):
    """2 x then 2 x lands on the lattice of 4 x with the same counts (the sums may differ by the extra rounding)."""
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    pts = _points("tiny")
    with NdtMatcher2D(cell_size=C0) as a, NdtMatcher2D(cell_size=2 * C0) as b, NdtMatcher2D(cell_size=4 * C0) as c2, \
            NdtMatcher2D(cell_size=4 * C0) as c4:
        a.set_target(pts[:, 0].copy(), pts[:, 1].copy())
        a.coarsen_into(b)
        b.coarsen_into(c2)
        a.coarsen_into(c4)
        h2, cells2 = R.parse(c2.save_map())
        h4, cells4 = R.parse(c4.save_map())
        assert (h2["width"], h2["height"]) == (h4["width"], h4["height"]) and np.array_equal(h2["origin"], h4["origin"])
        assert np.array_equal(cells2["n"], cells4["n"])


def test_coarsen_errors(gpu_lib):
    from gtsam_ndt_amd import _lib as L
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    lib = L.load()
    pts = _points("tiny")
    x, y = pts[:, 0].copy(), pts[:, 1].copy()
    with NdtMatcher2D(cell_size=C0) as src, NdtMatcher2D(cell_size=2 * C0) as dst:
        with pytest.raises(L.NdtError) as e:
            src.coarsen_into(dst)                                # no grid yet
        assert e.value.code == L.NDT_ERR_NO_TARGET
        src.set_target(x, y)
        for ratio in (1.0, 3.0, 8.0, 0.5, 2.0000001):
            with NdtMatcher2D(cell_size=ratio * C0) as bad:
                with pytest.raises(L.NdtError) as e:
                    src.coarsen_into(bad)
                assert e.value.code == L.NDT_ERR_INVALID_ARG and b"2 or 4" in lib.ndt_last_error()
        with pytest.raises(L.NdtError) as e:
            src.coarsen_into(src)
        assert e.value.code == L.NDT_ERR_INVALID_ARG
        assert lib.ndt2d_coarsen_map(None, dst._h) == L.NDT_ERR_INVALID_ARG
        assert lib.ndt2d_coarsen_map(src._h, None) == L.NDT_ERR_INVALID_ARG
        with NdtMatcher2D(cell_size=C0, overlap_grids=4) as four, NdtMatcher2D(cell_size=2 * C0, overlap_grids=4) as four2:
            four.set_target(x, y)
            for s, d in ((four, dst), (src, four2), (four, four2)):
                with pytest.raises(L.NdtError) as e:
                    s.coarsen_into(d)
                assert e.value.code == L.NDT_ERR_INVALID_ARG and b"overlapping" in lib.ndt_last_error()
        assert src.coarsen_into(dst) > 0                         # and none of this hurt either handle


def test_a_parent_beyond_the_cell_capacity(gpu_lib):
    """Four fine cells of 300 000 points each under one parent: 1.2 M > 2^20.  The coarse handle has no target afterwards."""
    from gtsam_ndt_amd import _lib as L
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    rng = np.random.default_rng(4)
    per = 300_000
    blocks = []
    for cx, cy in ((0.25, 0.25), (0.75, 0.25), (0.25, 0.75), (0.75, 0.75)):         # the four children of parent [0, 1)^2
        m = rng.integers(-200, 200, size=(per, 2))
        blocks.append(np.array([cx, cy]) + (2 * m + 1) * 2.0 ** -11)
    pts = np.vstack(blocks + [np.array([[-2.2, -2.2], [3.3, 3.3]])]).astype(np.float32)
    sx, sy = pts[:500, 0].copy(), pts[:500, 1].copy()
    with NdtMatcher2D(cell_size=C0) as src, NdtMatcher2D(cell_size=2 * C0) as dst:
        src.set_target(pts[:, 0].copy(), pts[:, 1].copy())
        dst.set_target(sx, sy)
        with pytest.raises(L.NdtError) as e:
            src.coarsen_into(dst)
        assert e.value.code == L.NDT_ERR_CAPACITY and b"2^20" in L.load().ndt_last_error()
        with pytest.raises(L.NdtError) as e:
            dst.align(sx, sy)
        assert e.value.code == L.NDT_ERR_NO_TARGET
        assert src.grid_info().n_valid >= 4                                          # src still holds its grid
