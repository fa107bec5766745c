"""ndt3d_merge_map / ndt3d_unmerge_map on the device: the 3D twin of test_gpu_merge_map.py (docs/ALGORITHM.md section 2.18):
the device must give the bytes of tests/map_merge_ref.py, and the destination must then be what a handle is after
ndt3d_load_map of those bytes.

Scenes and poses: merge_cases.py ("tiny" 9 x 8 x 7 voxels of 1 m with a single-point voxel and a degenerate block on which
the clamp acts - asserted; "wide" 40 x 30 x 12 voxels, 60 000 points; the source at half of the destination's voxel size in
one case each; all three angles in the general pose, and in "steep" and "near_gimbal" roll and pitch of 0.5 to 1.45 rad; no
ring in 3D, so "partly outside" means beyond the extent)."""
import numpy as np
import pytest

import map_coarsen_ref as R
import map_merge_ref as M
import merge_cases as MC

pytestmark = pytest.mark.gpu
DIM = 3

CASES = [("tiny", name, False) for name in ("identity", "shift", "general", "near_pi", "near_minus_pi", "partly_outside")] + \
        [("tiny", "general", True), ("wide", "general", False), ("wide", "partly_outside", False), ("wide", "near_pi", True)] + \
        [("tiny", name, False) for name in MC.TILTED] + [("tiny", "steep", True), ("wide", "near_gimbal", False)]


@pytest.mark.parametrize("scene,pose_name,half", CASES)
def test_merged_submap(gpu_lib, scene, pose_name, half):
    pose = MC.poses(DIM, scene)[pose_name]
    c_d = MC.C3 * (2 if half else 1)
    scan = MC.scan_of(DIM, scene, pose)
    blobs = []
    for run in range(2):                                            # two runs give equal bytes
        with MC.source(DIM, scene) as src, MC.destination(DIM, scene, c_d) as dst:
            src_blob, dst0 = src.save_map(), dst.save_map()
            want, want_out = M.map_merge_ref(dst0, src_blob, pose)
            out = dst.merge_map(src, pose)
            blob = dst.save_map()
            assert np.array_equal(blob, want)                       # the definition, byte for byte, header and n_points included
            assert out == want_out
            assert np.array_equal(src.save_map(), src_blob)         # src is unchanged
            blobs.append(blob)
            if run == 0:
                c = M.contributions(R.parse(src_blob)[0], R.parse(src_blob)[1], R.parse(dst0)[0], pose)
                if pose_name == "partly_outside":
                    total = int(c["n"].sum())
                    assert 0 < out < total and not np.any(c["on_ring"])
                elif pose_name in ("identity", "shift"):
                    assert out == 0
                if scene == "tiny" and pose_name == "general":
                    assert M.clamp_acted(dst0, src_blob, pose)
                if half:                                            # at least four source cells meet in one destination cell
                    assert np.bincount(c["cell"][c["cell"] >= 0]).max() >= 4
                MC.assert_is_a_loaded_handle(DIM, dst, blob, scan, MC.points(DIM, scene, seed=29))
    assert np.array_equal(blobs[0], blobs[1])


def test_merges_commute_and_unmerge_inverts(gpu_lib):
    _merges_commute_and_unmerge_inverts("general", "near_pi", "shift")


def test_merges_commute_and_unmerge_inverts_at_tilted_poses(gpu_lib):
    _merges_commute_and_unmerge_inverts("steep", "near_gimbal", "general")


def _merges_commute_and_unmerge_inverts(name_b, name_c, name_new):
    P = MC.poses(DIM, "tiny")
    tb, tc, t_new = P[name_b], P[name_c], P[name_new]
    scan = MC.scan_of(DIM, "tiny", tb)
    with MC.source(DIM, "tiny") as b, MC.source(DIM, "tiny", seed=29) as c, MC.destination(DIM, "tiny") as d1, \
            MC.destination(DIM, "tiny") as d2:
        a0 = d1.save_map()
        # merge(B); merge(C) = merge(C); merge(B)
        d1.merge_map(b, tb); d1.merge_map(c, tc)
        d2.merge_map(c, tc); d2.merge_map(b, tb)
        assert np.array_equal(d1.save_map(), d2.save_map())
        assert np.array_equal(d1.save_map(), M.map_merge_ref(M.map_merge_ref(a0, b.save_map(), tb)[0], c.save_map(), tc)[0])
        # back to the original, in the other order
        d1.unmerge_map(b, tb); d1.unmerge_map(c, tc)
        assert np.array_equal(d1.save_map(), a0)
        # merge(B, T); add scan; unmerge(B, T) = add scan alone
        out = d1.merge_map(b, tb)
        d1.add_target_points(*scan)
        assert d1.unmerge_map(b, tb) == out
        d2.unmerge_map(b, tb); d2.unmerge_map(c, tc)
        d2.add_target_points(*scan)
        assert np.array_equal(d1.save_map(), d2.save_map())
        d1.remove_target_points(*scan)
        assert np.array_equal(d1.save_map(), a0)
        # a loop closure moves B: unmerge(B, T_old); merge(B, T_new) = a merge at T_new into the original
        d1.merge_map(b, tb)
        d1.unmerge_map(b, tb); d1.merge_map(b, t_new)
        assert np.array_equal(d1.save_map(), M.map_merge_ref(a0, b.save_map(), t_new)[0])


def test_merge_drops_what_map_alignment_derived_from_the_old_grid(gpu_lib):
    """dst has served align_map on both sides before the merge; afterwards its map-to-map results are those of a fresh handle
    loaded from the merged blob (fails when the merge forgets grid_changed)."""
    import coarsen_cases as K
    pose = MC.poses(DIM, "tiny")["general"]
    with MC.source(DIM, "tiny") as src, MC.destination(DIM, "tiny") as dst, MC.source(DIM, "tiny", seed=29) as other, \
            MC.matcher(DIM, cell_size=MC.C3, eig_ratio=0.03) as fresh:
        before_t, before_s = dst.align_map(other, MC.zero(DIM)), other.align_map(dst, MC.zero(DIM))
        dst.merge_map(src, pose)
        fresh.load_map(dst.save_map())
        after_t, after_s = dst.align_map(other, MC.zero(DIM)), other.align_map(dst, MC.zero(DIM))
        K.same_result(after_t, fresh.align_map(other, MC.zero(DIM)))
        K.same_result(after_s, other.align_map(fresh, MC.zero(DIM)))
        assert after_t.score != before_t.score and after_s.score != before_s.score
        # ... and again after the unmerge
        dst.unmerge_map(src, pose)
        fresh.load_map(dst.save_map())
        K.same_result(dst.align_map(other, MC.zero(DIM)), fresh.align_map(other, MC.zero(DIM)))
        K.same_result(dst.align_map(other, MC.zero(DIM)), before_t)


def test_merge_refusals(gpu_lib):
    from gtsam_ndt_amd import _lib as L
    lib = L.load()
    pose = MC.poses(DIM, "tiny")["general"]
    cp = (L.C.c_double * 6)(*pose)

    def refused(d, s, p, code, word):
        with pytest.raises(L.NdtError) as e:
            d.merge_map(s, p)
        assert e.value.code == code and word in lib.ndt_last_error(), lib.ndt_last_error()
        with pytest.raises(L.NdtError) as e:
            d.unmerge_map(s, p)
        assert e.value.code == code and word in lib.ndt_last_error(), lib.ndt_last_error()

    with MC.source(DIM, "tiny") as src, MC.destination(DIM, "tiny") as dst:
        a0 = dst.save_map()
        for fn in (lib.ndt3d_merge_map, lib.ndt3d_unmerge_map):
            assert fn(None, src._h, cp, None) == L.NDT_ERR_INVALID_ARG and b"null" in lib.ndt_last_error()
            assert fn(dst._h, None, cp, None) == L.NDT_ERR_INVALID_ARG and b"null" in lib.ndt_last_error()
        refused(dst, dst, pose, L.NDT_ERR_INVALID_ARG, b"one handle")
        with MC.source(DIM, "tiny", c=2 * MC.C3) as coarse:
            refused(dst, coarse, pose, L.NDT_ERR_INVALID_ARG, b"cell_size")
        for j, v in enumerate((float("nan"), float("inf"), float("-inf"), float("nan"), float("inf"), float("nan"))):
            bad = list(pose)
            bad[j] = v
            refused(dst, src, bad, L.NDT_ERR_INVALID_ARG, b"finite")
        with MC.matcher(DIM, cell_size=MC.C3) as empty:
            refused(dst, empty, pose, L.NDT_ERR_NO_TARGET, b"no target")
            refused(empty, src, pose, L.NDT_ERR_NO_TARGET, b"no target")
        if lib.ndt_device_count() > 1:
            with MC.matcher(DIM, device=1, cell_size=MC.C3) as far:
                far.set_target(*MC.cols(MC.points(DIM, "tiny")))
                refused(dst, far, pose, L.NDT_ERR_INVALID_ARG, b"one device")
        assert np.array_equal(dst.save_map(), a0)                   # none of this touched dst
        with MC.destination(DIM, "tiny", own=False) as reserved:    # a reserved grid counts as a target
            assert reserved.merge_map(src, pose) == 0
            assert int(R.parse(reserved.save_map())[1]["n"].sum()) == len(MC.points(DIM, "tiny"))


def test_unmerge_of_what_was_never_merged(gpu_lib):
    from gtsam_ndt_amd import _lib as L
    pose = MC.poses(DIM, "tiny")["general"]
    scan = MC.scan_of(DIM, "tiny", pose)
    with MC.source(DIM, "tiny") as src, MC.destination(DIM, "tiny") as dst:
        with pytest.raises(L.NdtError) as e:
            dst.unmerge_map(src, pose)
        assert e.value.code == L.NDT_ERR_INVALID_ARG and b"not in the destination" in L.load().ndt_last_error()
        with pytest.raises(L.NdtError) as e:
            dst.align(*scan)
        assert e.value.code == L.NDT_ERR_NO_TARGET
        assert src.grid_info().n_valid > 0


def _forged_source(dim, c):
    """The blob of a 5-cell-wide grid whose centre cell holds 2^19 points: plausible sums that no test could afford to build."""
    ext = [5] * dim
    origin = np.array([-2.5 * c] * dim, dtype=np.float32)
    h, cells = R.parse(MC.empty_blob(dim, c, origin, ext))
    cells = cells.copy()
    k = sum(2 * int(np.prod(ext[:a])) for a in range(dim))
    n = 1 << 19
    cells["n"][k] = n
    cells["s"][k] = [n * 1000, -n * 2000, n * 500][:dim]
    diag = [j for j, (a, b) in enumerate(M.pairs_of(dim)) if a == b]
    for j in diag:
        cells["ss"][k][j] = n << 30
    h["n_points"] = n if dim == 2 else 0
    return R.pack(h, cells)


def test_a_destination_cell_beyond_the_capacity(gpu_lib):
    """One source cell of 2^19 points merged three times at the identity: 1.5 x 2^20 > 2^20 on the third merge."""
    from gtsam_ndt_amd import _lib as L
    forged = _forged_source(DIM, MC.C3)
    scan = MC.scan_of(DIM, "tiny", MC.zero(DIM))
    with MC.matcher(DIM, cell_size=MC.C3) as src, MC.destination(DIM, "tiny", own=False) as dst:
        src.load_map(forged)
        want = dst.save_map()
        for _ in range(2):
            want = M.map_merge_ref(want, forged, MC.zero(DIM))[0]
            assert dst.merge_map(src, MC.zero(DIM)) == 0
            assert np.array_equal(dst.save_map(), want)
        with pytest.raises(L.NdtError) as e:
            dst.merge_map(src, MC.zero(DIM))
        assert e.value.code == L.NDT_ERR_CAPACITY and b"2^20" in L.load().ndt_last_error()
        with pytest.raises(L.NdtError) as e:
            dst.align(*scan)
        assert e.value.code == L.NDT_ERR_NO_TARGET


def test_merge_through_the_map_pyramid(gpu_lib):
    """NdtMapPyramid3D.merge folds the other pyramid in level by level: every level holds the reference's bytes."""
    _merge_through_the_map_pyramid("general")


def test_merge_through_the_map_pyramid_at_a_steep_pose(gpu_lib):
    _merge_through_the_map_pyramid("steep")


def _merge_through_the_map_pyramid(pose_name):
    from gtsam_ndt_amd.matcher import NdtMapPyramid3D
    pose = MC.poses(DIM, "tiny")[pose_name]
    with MC.source(DIM, "tiny") as src, MC.destination(DIM, "tiny") as dst:
        src_blob, dst_blob = src.save_map(), dst.save_map()
    with NdtMapPyramid3D.from_blob(dst_blob) as pd, NdtMapPyramid3D.from_blob(src_blob) as ps:
        before = [(d.save_map(), s.save_map()) for d, s in zip(pd.levels, ps.levels)]
        assert len(before) > 1
        out = pd.merge(ps, pose)
        for m, (db, sb) in zip(pd.levels, before):
            assert np.array_equal(m.save_map(), M.map_merge_ref(db, sb, pose)[0])
        assert out == M.map_merge_ref(before[-1][0], before[-1][1], pose)[1]
