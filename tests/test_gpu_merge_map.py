"""ndt2d_merge_map / ndt2d_unmerge_map on the device: one submap folded into another at a pose from the per-cell sums alone
(docs/ALGORITHM.md section 2.18).  The contribution is float64 in a fixed operation order and integers from there on, so the
device must give the bytes of tests/map_merge_ref.py, header and n_points included, and the destination must then be what a
handle is after ndt2d_load_map of those bytes.

Scenes and poses: merge_cases.py ("tiny" 13 x 11 cells of 0.5 m with a single-point cell and a degenerate block on which
the clamp acts - asserted; "wide" 301 x 201 cells, 20 000 points, many workgroups; the source at half of the destination's
cell size in one case each)."""
import numpy as np
import pytest

import map_coarsen_ref as R
import map_merge_ref as M
import merge_cases as MC

pytestmark = pytest.mark.gpu
DIM = 2

CASES = [("tiny", name, False) for name in ("identity", "shift", "general", "near_pi", "near_minus_pi", "partly_outside")] + \
        [("tiny", "general", True), ("wide", "general", False), ("wide", "partly_outside", False), ("wide", "near_pi", True)]


@pytest.mark.parametrize("scene,pose_name,half", CASES)
def test_merged_submap(gpu_lib, scene, pose_name, half):
    pose = MC.poses(DIM, scene)[pose_name]
    c_d = MC.C2 * (2 if half else 1)
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
                    assert 0 < out < total and np.any(c["on_ring"]) and np.any((c["cell"] < 0) & ~c["on_ring"])
                elif pose_name in ("identity", "shift"):
                    assert out == 0
                if scene == "tiny" and pose_name == "general":
                    assert M.clamp_acted(dst0, src_blob, pose)
                if half:                                            # at least four source cells meet in one destination cell
                    assert np.bincount(c["cell"][c["cell"] >= 0]).max() >= 4
                MC.assert_is_a_loaded_handle(DIM, dst, blob, scan, MC.points(DIM, scene, seed=29))
    assert np.array_equal(blobs[0], blobs[1])


def test_merges_commute_and_unmerge_inverts(gpu_lib):
    P = MC.poses(DIM, "tiny")
    tb, tc, t_new = P["general"], P["near_pi"], P["shift"]
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
            MC.matcher(DIM, cell_size=MC.C2, eig_ratio=0.03) as fresh:
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
    cp = (L.C.c_double * 3)(*pose)

    def refused(d, s, p, code, word):
        with pytest.raises(L.NdtError) as e:
            d.merge_map(s, p)
        assert e.value.code == code and word in lib.ndt_last_error(), lib.ndt_last_error()
        with pytest.raises(L.NdtError) as e:
            d.unmerge_map(s, p)
        assert e.value.code == code and word in lib.ndt_last_error(), lib.ndt_last_error()

    with MC.source(DIM, "tiny") as src, MC.destination(DIM, "tiny") as dst:
        a0 = dst.save_map()
        for fn in (lib.ndt2d_merge_map, lib.ndt2d_unmerge_map):
            assert fn(None, src._h, cp, None) == L.NDT_ERR_INVALID_ARG and b"null" in lib.ndt_last_error()
            assert fn(dst._h, None, cp, None) == L.NDT_ERR_INVALID_ARG and b"null" in lib.ndt_last_error()
        refused(dst, dst, pose, L.NDT_ERR_INVALID_ARG, b"one handle")
        with MC.matcher(DIM, cell_size=MC.C2, overlap_grids=4) as four:
            four.set_target(*MC.cols(MC.points(DIM, "tiny")))
            refused(dst, four, pose, L.NDT_ERR_INVALID_ARG, b"overlapping")
            refused(four, src, pose, L.NDT_ERR_INVALID_ARG, b"overlapping")
        with MC.source(DIM, "tiny", c=2 * MC.C2) as coarse:
            refused(dst, coarse, pose, L.NDT_ERR_INVALID_ARG, b"cell_size")
        for bad in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, float("-inf"))):
            refused(dst, src, bad, L.NDT_ERR_INVALID_ARG, b"finite")
        with MC.matcher(DIM, cell_size=MC.C2) as empty:
            refused(dst, empty, pose, L.NDT_ERR_NO_TARGET, b"no target")
            refused(empty, src, pose, L.NDT_ERR_NO_TARGET, b"no target")
        if lib.ndt_device_count() > 1:
            with MC.matcher(DIM, device=1, cell_size=MC.C2) as far:
                far.set_target(*MC.cols(MC.points(DIM, "tiny")))
                refused(dst, far, pose, L.NDT_ERR_INVALID_ARG, b"one device")
        assert np.array_equal(dst.save_map(), a0)                   # none of this touched dst
        with MC.destination(DIM, "tiny", own=False) as reserved:    # a reserved grid counts as a target
            assert reserved.merge_map(src, pose) == 0
            assert reserved.grid_info().n_points == len(MC.points(DIM, "tiny"))


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
    forged = _forged_source(DIM, MC.C2)
    scan = MC.scan_of(DIM, "tiny", MC.zero(DIM))
    with MC.matcher(DIM, cell_size=MC.C2) as src, MC.destination(DIM, "tiny", own=False) as dst:
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
    """NdtMapPyramid2D.merge folds the other pyramid in level by level: every level holds the reference's bytes."""
    from gtsam_ndt_amd.matcher import NdtMapPyramid2D
    pose = MC.poses(DIM, "tiny")["general"]
    with MC.source(DIM, "tiny") as src, MC.destination(DIM, "tiny") as dst:
        src_blob, dst_blob = src.save_map(), dst.save_map()
    with NdtMapPyramid2D.from_blob(dst_blob) as pd, NdtMapPyramid2D.from_blob(src_blob) as ps:
        before = [(d.save_map(), s.save_map()) for d, s in zip(pd.levels, ps.levels)]
        assert len(before) > 1
        out = pd.merge(ps, pose)
        for m, (db, sb) in zip(pd.levels, before):
            assert np.array_equal(m.save_map(), M.map_merge_ref(db, sb, pose)[0])
        assert out == M.map_merge_ref(before[-1][0], before[-1][1], pose)[1]
