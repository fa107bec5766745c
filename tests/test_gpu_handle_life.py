"""One long-lived handle, and its long-lived partner for the map-to-map calls, walked through a whole life: every mutator
(set_target, reserve, add, remove, merge, unmerge, load, coarsen; a removal and a merge that fail) and every query family
in the seeded order of tests/handle_life.py, about 80 calls on the same two handles.  What a handle carries from call to
call - the ping-pong halves of the sorted build, build_seq / last_ntile, the map-to-map caches, call_seq, the async lanes,
scratch that grew at an earlier call, sixteen cached launch graphs - is checked through what it answers:

  after every mutator   save_map() is HandleModel.blob() byte for byte (header and n_points included), grid_info().n_valid
                        and the returned n_outside are the model's integers; a predicted failure returns the predicted
                        status and leaves NDT_ERR_NO_TARGET behind, for the queries that follow it too;
  after every query     the answer is bit for bit the answer of a FRESH handle of the same parameters, created for that
                        step, that loaded model.blob() (ndt*_load_map is pinned bit for bit to ndt*_set_target by
                        tests/test_gpu_map_io.py) - pose, H, g, score, n_hit, iterations, status, score lists, hit lists,
                        per-point classes and selected points, compared as bytes.  A run of align_async calls is compared
                        with the fresh handle's plain align of the run's last scan ("ndt2d_align_finish returns the last
                        call's result", "bit-identical result": include/ndt_hip.h).

Bitwise equality between two handles is what the contract promises for every family here (fixed reduction orders:
tests/test_determinism.py; the multi and async calls "bit for bit" their single call), so no tolerance appears in this file.

Handle `who` of a life with seed s runs with fixed_iterations = 3 when (s + who) is odd and to convergence otherwise, so
both kinds of loop live on a long-lived handle in each dimension, and a map-to-map call crosses the two.

The overlap_grids = 4 run (2D): the exact-blob model does not cover the four grids; there the truth is a fresh handle
rebuilt from the points that should be in the map (reserve of the same box + adds), blobs compared byte for byte.

Wall time on one MI355X, fresh handles and the model's replay included: test_one_life 0.80 s (2D, seed 0, which also
generates the schedules' shared inputs), 0.36 s (2D, seed 1), 0.37 s and 0.38 s (3D); test_one_life_with_overlapping_grids
0.11 s; loading the library for the first test of the file 1.5 s."""
import numpy as np
import pytest

import handle_life as HL

pytestmark = pytest.mark.gpu


def _matcher(dim, **kw):
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D
    kw.setdefault("cell_size", HL.CELL[dim])
    return (NdtMatcher2D if dim == 2 else NdtMatcher3D)(**kw)


def _params(seed, who):
    return {"fixed_iterations": 3} if (seed + who) % 2 else {}


def _cols(pts):
    pts = np.asarray(pts, dtype=np.float32)
    return [np.ascontiguousarray(pts[:, a]) for a in range(pts.shape[1])]


def _dev(pts):
    import torch
    return [torch.from_numpy(c).cuda() for c in _cols(pts)]


# ---- results as lists of numpy arrays, compared as bytes ------------------------------------------------------------------
def _flat(x):
    from gtsam_ndt_amd.matcher import AlignResult, AlignResult3D, PointFit
    from gtsam_ndt_amd.search import SearchHit
    if isinstance(x, (AlignResult, AlignResult3D)):
        return [np.asarray(x.pose, np.float64), x.H, x.g, np.float64(x.score), np.int64(x.iterations), np.int64(x.n_hit), np.int64(x.status)]
    if isinstance(x, SearchHit):
        return [np.asarray(x.pose, np.float64), np.float64(x.score), np.int64(x.index)]
    if isinstance(x, PointFit):
        return [_flat(x.m), _flat(x.cls), np.int64([x.n_invalid, x.n_miss, x.n_misfit, x.n_fit, x.n_selected])]
    if isinstance(x, (list, tuple)):
        return [_flat(v) for v in x]
    if hasattr(x, "data_ptr"):
        return x.cpu().numpy()
    return x if x is None else np.asarray(x)


def _assert_same(got, want, where):
    if isinstance(want, list):
        assert isinstance(got, list) and len(got) == len(want), where
        for j, (u, v) in enumerate(zip(got, want)):
            _assert_same(u, v, f"{where}[{j}]")
    elif want is None:
        assert got is None, where
    else:
        assert got.dtype == want.dtype and got.shape == want.shape, where
        np.testing.assert_array_equal(np.ascontiguousarray(got).reshape(-1).view(np.uint8),
                                      np.ascontiguousarray(want).reshape(-1).view(np.uint8), err_msg=where)


# ---- one step on real handles ---------------------------------------------------------------------------------------------
def _mutate(dim, h, step):
    """-> (status, n_outside)"""
    from gtsam_ndt_amd import _lib as L
    op = step[0]
    try:
        out = None
        if op == "set_target":
            h.set_target(*_cols(step[2]))
        elif op == "reserve":
            lo, hi = [float(v) for v in step[2]], [float(v) for v in step[3]]
            h.reserve_target(*lo, *hi) if dim == 2 else h.reserve_target(lo, hi)
        elif op in ("add", "remove"):
            fn = h.add_target_points if op == "add" else h.remove_target_points
            out = fn(*_cols(step[2])) if step[3] is None else fn(*_dev(step[2]), pose=tuple(step[3]))
        elif op in ("merge", "unmerge"):
            with _matcher(dim) as src:
                src.load_map(step[2])
                out = (h.merge_map if op == "merge" else h.unmerge_map)(src, tuple(step[3]))
        elif op == "load":
            h.load_map(step[2])
        elif op == "coarsen_from":
            with _matcher(dim, cell_size=HL.CELL[dim] / int(step[3])) as fine:
                fine.set_target(*_cols(step[2]))
                fine.coarsen_into(h)
        else:
            raise KeyError(op)
        return L.NDT_OK, out
    except L.NdtError as e:
        return e.code, None


def _query(step, tgt, src, plain_async=False):
    op = step[0]
    if op == "align":
        return tgt.align(*_dev(step[2]), tuple(step[3]))
    if op == "align_host":
        return tgt.align(*_cols(step[2]), tuple(step[3]))
    if op == "align_async":
        if plain_async:
            return tgt.align(*_dev(step[2][-1]), tuple(step[3][-1]))
        scans = [_dev(s) for s in step[2]]                          # every call's arrays stay valid until finish returns
        for s, init in zip(scans, step[3]):
            tgt.align_async(*s, tuple(init))
        return tgt.finish()
    if op == "align_trace":
        return tgt.align_trace(*_cols(step[2]), tuple(step[3]))
    if op == "evaluate":
        return tgt.evaluate(*(_cols(step[2]) if len(step[2]) <= 65 else _dev(step[2])), tuple(step[3]))
    if op == "multi_start":
        return tgt.align_multi_start(*_dev(step[2]), step[3])
    if op == "multi_scan":
        return tgt.align_multi_scan([tuple(_dev(s)) for s in step[2]], step[3])
    if op == "score_poses":
        return tgt.score_poses(*_cols(step[2]), step[3])
    if op == "score_particles":
        import torch
        return tgt.score_particles(*_dev(step[2]), torch.from_numpy(np.ascontiguousarray(step[3])).cuda(), with_hits=True)
    if op == "search_align":
        return tgt.search_align(*_cols(step[2]), step[3], step[4], step[5], k=step[6])
    if op == "fit_points":
        return tgt.fit_points(*_cols(step[2]), tuple(step[3]), step[4])
    if op == "select_points":
        return tgt.select_points(*_cols(step[2]), tuple(step[3]), step[4])
    if op == "align_map":
        return tgt.align_map(src, tuple(step[2]))
    if op == "align_map_multi":
        return tgt.align_map_multi(src, step[2])
    if op == "score_map_poses":
        return tgt.score_map_poses(src, step[2], with_hits=True)
    if op == "search_align_map":
        return tgt.search_align_map(src, step[2], step[3], step[4], k=step[5])
    raise KeyError(op)


def _expect_no_target(call):
    from gtsam_ndt_amd import _lib as L
    with pytest.raises(L.NdtError) as e:
        call()
    assert e.value.code == L.NDT_ERR_NO_TARGET


@pytest.mark.parametrize("dim,seed", [(2, 0), (2, 1), (3, 0), (3, 1)])
def test_one_life(gpu_lib, dim, seed):
    from gtsam_ndt_amd import _lib as L
    life = HL.Life(dim)
    seen = {"mutators": 0, "failures": 0, "no_target": 0, "queries": 0, "hits": 0}
    with _matcher(dim, **_params(seed, 0)) as h0, _matcher(dim, **_params(seed, 1)) as h1:
        handles = (h0, h1)

        def fresh(who):
            m = _matcher(dim, **_params(seed, who))
            m.load_map(life.model[who].blob())
            if life.neighbourhood[who] != 1:
                m.set_neighbourhood(life.neighbourhood[who])
            return m

        for j, step in enumerate(HL.schedule(dim, seed)):
            op, who = step[0], step[1]
            where = f"step {j}: {op} on handle {who}"
            pred = life.apply(step)
            h, model = handles[who], life.model[who]
            if pred["kind"] == "setting":
                h.set_neighbourhood(int(step[2]))
                assert h.neighbourhood == int(step[2])
            elif pred["kind"] == "mutator":
                status, n_outside = _mutate(dim, h, step)
                assert status == pred["status"], where
                seen["mutators"] += 1
                if status != L.NDT_OK:
                    _expect_no_target(h.grid_info)
                    seen["failures"] += 1
                    continue
                assert n_outside == pred["n_outside"], where
                np.testing.assert_array_equal(h.save_map(), model.blob(), err_msg=where)
                gi = h.grid_info()
                assert gi.n_valid == model.n_valid(), where
                if dim == 2:
                    assert gi.n_points == model.n_points(), where
            elif pred["status"] == L.NDT_ERR_NO_TARGET:
                _expect_no_target(lambda: _query(step, h, handles[1 - who]))
                seen["no_target"] += 1
            else:
                res = _query(step, h, handles[1 - who])
                got = _flat(res)
                seen["queries"] += 1
                if op in ("align", "align_host", "align_async", "align_map"):
                    n = len(step[2][-1] if op == "align_async" else step[2]) if op != "align_map" else 0
                    print(f"  step {j} {op} on {who}: {n} points, status {res.status}, {res.iterations} iterations, n_hit {res.n_hit}")
                    seen["hits"] += res.n_hit >= 100
                with fresh(who) as ft:
                    if op in HL.MAP_QUERIES:
                        with fresh(1 - who) as fs:
                            want = _flat(_query(step, ft, fs))
                    else:
                        want = _flat(_query(step, ft, None, plain_async=True))
                _assert_same(got, want, where)
    print(f"life {dim}D seed {seed}: {seen}")
    # the walk did what the schedule says, and its alignments met their maps
    assert seen["mutators"] >= 30 and seen["failures"] == 4 and seen["no_target"] >= 8 and seen["queries"] >= 32 and seen["hits"] >= 1, seen


def test_one_life_with_overlapping_grids(gpu_lib):
    """overlap_grids = 4: after every mutator the long-lived handle's four grids are, byte for byte, those of a handle
    rebuilt from the points that should be in the map; every query answers as that handle does."""
    inside = []                                                     # (points, pose) in the map
    box = None

    def rebuilt():
        m = _matcher(2, overlap_grids=4)
        _mutate(2, m, ("reserve", 0) + box)
        for pts, pose in inside:
            _mutate(2, m, ("add", 0, pts, pose))
        return m

    with _matcher(2, overlap_grids=4) as h:
        for j, step in enumerate(HL.short_schedule(0)):
            op = step[0]
            where = f"step {j}: {op}"
            if op in HL.POINT_QUERIES:
                got = _flat(_query(step, h, None))
                with rebuilt() as ref:
                    want = _flat(_query(step, ref, None, plain_async=True))
                _assert_same(got, want, where)
                continue
            if op == "reserve":
                box, inside = (step[2], step[3]), []
            elif op == "add":
                inside.append((step[2], step[3]))
            else:
                k = next(k for k, (pts, pose) in enumerate(inside) if pts is step[2] and pose is step[3])
                inside.pop(k)
            status, n_outside = _mutate(2, h, step)
            assert status == 0, where
            with rebuilt() as ref:
                np.testing.assert_array_equal(h.save_map(), ref.save_map(), err_msg=where)
                a, b = h.grid_info(), ref.grid_info()
                assert (a.n_valid, a.n_points) == (b.n_valid, b.n_points), where
