"""ndt3d_coarsen_map on the device: the 3D twin of test_gpu_coarsen_map.py (docs/ALGORITHM.md section 2.17).

Scenes: "tiny" 9 x 7 x 5 voxels of 0.5 m (coarsen_cases.lattice_cloud: coordinates on a 2^-11 lattice, origin cells negative
and no multiple of f, interior extents no multiple of f, occupied voxels next to the ring on all six sides) plus one voxel
of five identical points alone in its parent, off that lattice, so that the roundings and the degenerate-cell clamp act
(asserted); "fixture" the 4 096 target points of tests/golden/ndt3d_small.npz at 1 m voxels (44 x 44 x 9).  Both paths bin
every point alike on both scenes - asserted before anything is compared with a build at the coarse cell."""
import os

import numpy as np
import pytest

import coarsen_cases as K
import map_coarsen_ref as R

pytestmark = pytest.mark.gpu

GOLD3 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ndt3d_small.npz")
TINY = ((-3, -1, -1), (9, 7, 5))
CELL = {"tiny": 0.5, "fixture": 1.0}
ZERO = (0.0,) * 6
_cache = {}


def _points(scene):
    if scene not in _cache:
        if scene == "tiny":
            pts = K.lattice_cloud(23, TINY[0], TINY[1], 0.5, 400, ((0.0, 0.0, 0.0), (2.0, 2.0, 2.0)))
            p = np.array(CLUSTER)
            pts = np.vstack([pts, np.repeat(p[None, :], 5, axis=0)]).astype(np.float32)
        else:
            d = np.load(GOLD3)
            pts = np.stack([d["tx"], d["ty"], d["tz"]], axis=1).astype(np.float32)
        _cache[scene] = pts
    return _cache[scene]


CLUSTER = (1.8 + 2.0 ** -23, 1.8 + 5 * 2.0 ** -23, 1.3 + 3 * 2.0 ** -23)


def _scan(pts, n=400):
    """A small scan of the scene: some of its points, a few centimetres off."""
    rng = np.random.default_rng(2)
    q = pts[rng.choice(len(pts), size=min(n, len(pts)), replace=False)].astype(np.float64)
    cs, sn = np.cos(0.004), np.sin(0.004)
    x = cs * q[:, 0] - sn * q[:, 1] + 0.03
    y = sn * q[:, 0] + cs * q[:, 1] - 0.02
    return x.astype(np.float32), y.astype(np.float32), (q[:, 2] + 0.01).astype(np.float32)


@pytest.mark.parametrize("f", [2, 4])
@pytest.mark.parametrize("scene", ["tiny", "fixture"])
def test_coarsened_submap3d(gpu_lib, scene, f):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    pts, c = _points(scene), CELL[scene]
    if scene == "tiny":
        K.assert_lattice_is_awkward(TINY[0], TINY[1], f)
    assert K.bins_alike(pts, c, f)
    x, y, z = (pts[:, a].copy() for a in range(3))
    scan = _scan(pts)
    coarse = dict(cell_size=f * c, eig_ratio=0.03)
    with NdtMatcher3D(cell_size=c) as src, NdtMatcher3D(**coarse) as dst, NdtMatcher3D(**coarse) as direct, \
            NdtMatcher3D(**coarse) as loaded, NdtMatcher3D(**coarse) as other:
        src.set_target(x, y, z)
        fine_blob = src.save_map()
        if scene == "tiny":
            assert K.clamp_was_needed(fine_blob, f)
        dst.set_target(*scan)                                    # stale records of another map
        n_valid = src.coarsen_into(dst)
        blob = dst.save_map()
        # the definition, byte for byte, header included
        assert np.array_equal(blob, R.map_coarsen_ref(fine_blob, f))
        # against a build from the same points at the coarse voxel
        direct.set_target(x, y, z)
        worst = R.check_against_direct(blob, direct.save_map(), f)
        print(f"{scene} f={f}: largest |coarsened - direct| first sums {worst[0]}, second sums {worst[1]}")
        idst, idir = dst.grid_info(), direct.grid_info()
        assert (idst.ox, idst.oy, idst.oz, idst.width, idst.height, idst.depth) == (idir.ox, idir.oy, idir.oz, idir.width, idir.height, idir.depth)
        assert n_valid == idst.n_valid and n_valid > 0
        # dst is what a handle is after load_map
        loaded.load_map(blob)
        K.same_grid(dst, loaded)
        K.same_result(dst.align(*scan, ZERO), loaded.align(*scan, ZERO))
        other.set_target(*scan)
        K.same_result(dst.align_map(other, ZERO), loaded.align_map(other, ZERO))
        K.same_result(other.align_map(dst, ZERO), other.align_map(loaded, ZERO))
        # it takes points, and gives them back
        out_add = dst.add_target_points(*scan)
        assert not np.array_equal(dst.save_map(), blob)
        assert dst.remove_target_points(*scan) == out_add
        assert np.array_equal(dst.save_map(), blob)
        # src is unchanged
        assert np.array_equal(src.save_map(), fine_blob)


def test_ring_voxels_that_hold_points_are_kept(gpu_lib):
    """A 3D grid has no empty-ring contract: ndt3d_add_target_points bins into the ring voxels of a reserved extent, and
    coarsening keeps those sums where the lattice puts them - the reference, which knows no ring, gives the same bytes, and
    no point is lost."""
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    pts = _points("tiny")
    lo, hi = pts.min(axis=0), pts.max(axis=0)
    with NdtMatcher3D(cell_size=0.5) as src, NdtMatcher3D(cell_size=1.0) as dst:
        src.reserve_target(tuple(float(v) for v in lo), tuple(float(v) for v in hi))
        info = src.grid_info()
        ring = np.array([[info.ox + 0.25, info.oy + 0.25, info.oz + 0.25]] * 4 +
                        [[info.ox + (info.width - 0.5) * 0.5, info.oy + (info.height - 0.5) * 0.5, info.oz + (info.depth - 0.5) * 0.5]] * 3, dtype=np.float32)
        allp = np.vstack([pts, ring]).astype(np.float32)
        assert src.add_target_points(allp[:, 0].copy(), allp[:, 1].copy(), allp[:, 2].copy()) == 0
        fine_blob = src.save_map()
        _, cells = R.parse(fine_blob)
        assert cells["n"][0] == 4 and cells["n"][-1] == 3
        src.coarsen_into(dst)
        blob = dst.save_map()
        assert np.array_equal(blob, R.map_coarsen_ref(fine_blob, 2))
        assert int(R.parse(blob)[1]["n"].sum()) == len(allp)


def test_coarsen_errors3d(gpu_lib):
    from gtsam_ndt_amd import _lib as L
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    lib = L.load()
    pts = _points("tiny")
    x, y, z = (pts[:, a].copy() for a in range(3))
    with NdtMatcher3D(cell_size=0.5) as src, NdtMatcher3D(cell_size=1.0) as dst:
        with pytest.raises(L.NdtError) as e:
            src.coarsen_into(dst)                                # no grid yet
        assert e.value.code == L.NDT_ERR_NO_TARGET
        src.set_target(x, y, z)
        for ratio in (1.0, 3.0, 8.0):
            with NdtMatcher3D(cell_size=ratio * 0.5) as bad:
                with pytest.raises(L.NdtError) as e:
                    src.coarsen_into(bad)
                assert e.value.code == L.NDT_ERR_INVALID_ARG and b"2 or 4" in lib.ndt_last_error()
        with pytest.raises(L.NdtError) as e:
            src.coarsen_into(src)
        assert e.value.code == L.NDT_ERR_INVALID_ARG
        assert lib.ndt3d_coarsen_map(None, dst._h) == L.NDT_ERR_INVALID_ARG
        assert lib.ndt3d_coarsen_map(src._h, None) == L.NDT_ERR_INVALID_ARG
        assert src.coarsen_into(dst) > 0                         # and none of this hurt either handle


def test_a_parent_voxel_beyond_the_cell_capacity(gpu_lib):
    """Eight voxels of 150 000 points each under one parent: 1.2 M > 2^20.  The coarse handle has no target afterwards."""
    from gtsam_ndt_amd import _lib as L
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    rng = np.random.default_rng(4)
    per = 150_000
    blocks = []
    for k in range(8):                                           # the eight children of parent [0, 1)^3
        centre = np.array([0.25 + 0.5 * (k & 1), 0.25 + 0.5 * ((k >> 1) & 1), 0.25 + 0.5 * (k >> 2)])
        blocks.append(centre + (2 * rng.integers(-200, 200, size=(per, 3)) + 1) * 2.0 ** -11)
    pts = np.vstack(blocks + [np.array([[-2.2, -2.2, -1.2], [3.3, 3.3, 2.3]])]).astype(np.float32)
    scan = tuple(pts[:500, a].copy() for a in range(3))
    with NdtMatcher3D(cell_size=0.5) as src, NdtMatcher3D(cell_size=1.0) as dst:
        src.set_target(*(pts[:, a].copy() for a in range(3)))
        dst.set_target(*scan)
        with pytest.raises(L.NdtError) as e:
            src.coarsen_into(dst)
        assert e.value.code == L.NDT_ERR_CAPACITY and b"2^20" in L.load().ndt_last_error()
        with pytest.raises(L.NdtError) as e:
            dst.align(*scan)
        assert e.value.code == L.NDT_ERR_NO_TARGET
        assert src.grid_info().n_valid >= 8                      # src still holds its grid
