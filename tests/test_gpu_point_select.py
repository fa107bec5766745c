"""ndt2d/ndt3d_select_points_dev: the deterministic compaction behind the per-point fit, and the loop it is for.

Sizes: 1, 2, the wave (63, 64, 65), the workgroup (255, 256, 257) and 2^k - 1, 2^k, 2^k + 1 for k = 10 .. 13 - around
the 1024-point tile (kFitTile of csrc/ndt_point_fit.hpp) and up to eight tiles and one point.  Expectations come from the
classes the device returned (pinned to the reference by test_gpu_point_fit.py) and from numpy: the index equals
flatnonzero of the mask and is strictly ascending, the coordinates are the input's bits at those indices, the tails past
n_selected keep their sentinel, n_selected and the four counts are exact, two calls give identical bytes, and null or
non-null m / class arrays give the same summary."""
import numpy as np
import pytest

import point_fit_cases as PC
import point_fit_ref as F

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257] + [2 ** k + d for k in range(10, 14) for d in (-1, 0, 1)]
SENTINEL = np.float32(-12345.5)
FIT_MISS = (1 << F.FIT) | (1 << F.MISS)


@pytest.fixture(scope="module")
def scenes(gpu_lib):
    """Per dimension: a matcher of the fixture's target, and ONE mixed scan of the largest size with its device
    classes; every size below is a prefix of it."""
    out = {}
    for dim in (2, 3):
        m = PC.matcher(dim)
        rec = F.records_of(m)
        fx = PC.fixture(dim)
        pose = fx["final_pose"]
        coords, _ = PC.mixed_scan(rec, fx["source"], pose, max(SIZES))
        cls = m.fit_points(*coords, pose, PC.MAX_M[dim]).cls
        assert set(np.unique(cls)) == {0, 1, 2, 3}
        out[dim] = dict(m=m, rec=rec, pose=pose, coords=coords, dev=PC.dev(coords), cls=cls, max_m=PC.MAX_M[dim])
    yield out
    for s in out.values():
        s["m"].close()


def _select(m, dcoords, pose, max_m, keep, with_index=True):
    """One raw call into sentinel-filled outputs -> (out arrays, index array, summary tuple)."""
    import torch
    n = dcoords[0].numel()
    out = [torch.full((n,), float(SENTINEL), dtype=torch.float32, device="cuda") for _ in dcoords]
    index = torch.full((n,), -7, dtype=torch.int32, device="cuda") if with_index else None
    st, fit = PC.raw_select(m, dcoords, pose, max_m, keep, out, index)
    assert st == 0
    return [o.cpu().numpy() for o in out], (index.cpu().numpy() if with_index else None), PC.fit_tuple(fit)


def _assert_selection(coords, cls, keep, out, index, summary):
    """coords / cls: numpy, of the scan that was selected from."""
    n = len(cls)
    want = np.flatnonzero(F.keep_mask(cls, keep))
    c = F.counts(cls)
    assert summary == (c["n_invalid"], c["n_miss"], c["n_misfit"], c["n_fit"], len(want))
    k = len(want)
    if index is not None:
        assert np.array_equal(index[:k].astype(np.int64), want) and np.all(np.diff(index[:k]) > 0)
        assert np.all(index[k:] == -7)
    for a, o in enumerate(out):
        assert o[:k].tobytes() == coords[a][want].tobytes()                     # bit for bit, NaN payloads included
        assert np.all(o[k:] == SENTINEL) and len(o) == n


@pytest.mark.parametrize("n", SIZES)
def test_sizes(scenes, n):
    s = scenes[2]
    m, pose, max_m = s["m"], s["pose"], s["max_m"]
    coords = tuple(c[:n] for c in s["coords"])
    dcoords = tuple(c[:n].contiguous() for c in s["dev"])
    cls = s["cls"][:n]
    out, index, summary = _select(m, dcoords, pose, max_m, FIT_MISS)
    _assert_selection(coords, cls, FIT_MISS, out, index, summary)
    out2, index2, summary2 = _select(m, dcoords, pose, max_m, FIT_MISS)
    assert summary2 == summary and index2.tobytes() == index.tobytes()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out, out2))
    # without an index array, and the fit call with and without its arrays: the same summary
    out3, _, summary3 = _select(m, dcoords, pose, max_m, FIT_MISS, with_index=False)
    assert summary3 == summary and all(a.tobytes() == b.tobytes() for a, b in zip(out, out3))
    import torch
    dm = torch.empty(n, dtype=torch.float32, device="cuda")
    dc = torch.empty(n, dtype=torch.uint8, device="cuda")
    fits = [PC.raw_fit(m, dcoords, pose, max_m, a, b) for a, b in ((None, None), (dm, None), (None, dc), (dm, dc))]
    assert all(st == 0 for st, _ in fits)
    assert len({PC.fit_tuple(f) for _, f in fits}) == 1 and PC.fit_tuple(fits[0][1]) == summary[:4] + (0,)
    assert dc.cpu().numpy().tobytes() == cls.tobytes()


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("keep", range(1, 16))
def test_every_mask_on_a_mixed_scan(scenes, dim, keep):
    s = scenes[dim]
    n = 5000 if dim == 2 else 3001
    coords = tuple(c[:n] for c in s["coords"])
    dcoords = tuple(c[:n].contiguous() for c in s["dev"])
    out, index, summary = _select(s["m"], dcoords, s["pose"], s["max_m"], keep)
    _assert_selection(coords, s["cls"][:n], keep, out, index, summary)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("where", ["first", "last", "none", "all"])
def test_kept_points_in_one_tile_none_and_all(scenes, dim, where):
    """Five tiles; the scan's points outside one tile are far from the map (misses), and FIT is kept: the kept points are
    all in the first tile, or all in the last.  none: a scan of misses only.  all: every class kept."""
    s = scenes[dim]
    m, pose, max_m = s["m"], s["pose"], s["max_m"]
    n, tile = 5 * 1024 - 3, 1024
    coords = [c[:n].copy() for c in s["coords"]]
    lo, hi = {"first": (0, tile), "last": (4 * tile, n), "none": (0, 0), "all": (0, n)}[where]
    outside = np.ones(n, bool)
    outside[lo:hi] = False
    for a in range(dim):
        coords[a][outside] = np.float32(5.0e4 + 10.0 * a)
    keep = 15 if where == "all" else 1 << F.FIT
    got = m.fit_points(*coords, pose, max_m)
    assert np.all(got.cls[outside] == F.MISS)
    out, index, summary = _select(m, PC.dev(coords), pose, max_m, keep)
    _assert_selection(coords, got.cls, keep, out, index, summary)
    k = summary[4]
    if where == "none":
        assert k == 0
    elif where == "all":
        assert k == n
    else:
        assert k > 100 and index[0] >= lo and index[k - 1] < hi


@pytest.mark.parametrize("dim", [2, 3])
def test_matcher_select_points_in_and_out_kinds(scenes, dim):
    """select_points of the Python matcher: numpy in, numpy out; tensors in, tensors out; trimmed to n_selected."""
    import torch
    s = scenes[dim]
    n = 3000
    coords = tuple(c[:n] for c in s["coords"])
    want = np.flatnonzero(F.keep_mask(s["cls"][:n], FIT_MISS))
    sel, idx, fit = s["m"].select_points(*coords, s["pose"], s["max_m"])
    assert all(isinstance(c, np.ndarray) and c.dtype == np.float32 for c in sel) and np.array_equal(idx, want)
    assert fit.n_selected == len(want) and fit.m is None and fit.cls is None
    dsel, didx, dfit = s["m"].select_points(*PC.dev(coords), s["pose"], s["max_m"], keep=FIT_MISS)
    assert all(isinstance(c, torch.Tensor) and c.is_cuda for c in dsel) and np.array_equal(didx.cpu().numpy(), want)
    for a in range(dim):
        assert sel[a].tobytes() == coords[a][want].tobytes() == dsel[a].cpu().numpy().tobytes()
    only_fit = s["m"].select_points(*coords, s["pose"], s["max_m"], keep="fit")[1]
    assert np.array_equal(only_fit, np.flatnonzero(s["cls"][:n] == F.FIT))
    assert dfit.n_hit == dfit.n_fit + dfit.n_misfit and 0.0 < dfit.fitness < 1.0


def test_selection_at_a_steep_pose_3d(scenes):
    """The 3D scan seen from a frame rolled 0.7 and pitched -0.5 rad (point_fit_cases.steep_scene): the classes are the
    reference's within its excuses, the selection is flatnonzero of the device's own classes, the input's bits in scan
    order, through the raw call and through the matcher."""
    s = scenes[3]
    m, rec, max_m = s["m"], s["rec"], s["max_m"]
    source, pose = PC.steep_scene(PC.fixture(3))
    n = 3001
    coords, _ = PC.mixed_scan(rec, source, pose, n)
    got = m.fit_points(*coords, pose, max_m)
    fig, fails = F.compare(F.fit_ref(rec, coords, pose, max_m), got.m, got.cls, max_m)
    assert not fails and set(np.unique(got.cls)) == {0, 1, 2, 3}, (fails, fig)
    for keep in (FIT_MISS, 1 << F.FIT, 15):
        out, index, summary = _select(m, PC.dev(coords), pose, max_m, keep)
        _assert_selection(coords, got.cls, keep, out, index, summary)
    want = np.flatnonzero(F.keep_mask(got.cls, FIT_MISS))
    sel, idx, fit = m.select_points(*coords, pose, max_m)
    assert np.array_equal(idx, want) and fit.n_selected == len(want) > 1000 and np.all(np.diff(idx) > 0)
    for a in range(3):
        assert sel[a].tobytes() == coords[a][want].tobytes()


@pytest.mark.parametrize("dim", [2, 3])
def test_the_loop_it_is_for(gpu_lib, dim):
    """The map is built from the target; the scan is the fixture's source plus 200 points moved 0.25 m along the minor
    axis of the cell they hit, every one of which the REFERENCE classes as not fitting before the device is asked - here
    all MISFIT, with the tolerance to spare: a moved point that leaves the mapped cells altogether is a MISS, and a
    selection of fit | miss keeps misses by design (they extend the map), so the 200 are taken among the hits whose
    moved image stays in a valid cell.  select_points(fit | miss) returns none of them; adding the selection leaves save_map() byte-equal to adding the
    numpy-filtered scan on a second handle; removing the same selection restores the original blob."""
    fx = PC.fixture(dim)
    pose, max_m = fx["final_pose"], PC.MAX_M[dim]
    with PC.matcher(dim) as m, PC.matcher(dim) as other:
        rec = F.records_of(m)
        src, moved = PC.displaced_outliers(rec, fx["source"], pose, 200, misfit_only=True)
        n0 = len(fx["source"][0])
        scan = tuple(np.concatenate([fx["source"][a], moved[:, a]]) for a in range(dim))
        ref = F.fit_ref(rec, scan, pose, max_m)
        assert np.all(ref["cls"][n0:] == F.MISFIT) and not ref["near"][n0:].any()
        assert np.all(ref["m"][n0:] - max_m > ref["tol"][n0:])
        before = m.save_map().tobytes()
        assert other.save_map().tobytes() == before
        dscan = PC.dev(scan)
        sel, idx, fit = m.select_points(*dscan, pose, max_m, keep=("fit", "miss"))
        idx = idx.cpu().numpy()
        assert fit.n_selected == len(idx) > 500 and not (idx >= n0).any()
        # the second handle gets the numpy-filtered scan
        cls = other.fit_points(*scan, pose, max_m).cls
        mask = (cls == F.FIT) | (cls == F.MISS)
        assert np.array_equal(np.flatnonzero(mask), idx)
        out_a = m.add_target_points(*sel, pose=pose)
        out_b = other.add_target_points(*PC.dev(tuple(c[mask] for c in scan)), pose=pose)
        merged = m.save_map().tobytes()
        assert out_a == out_b and merged == other.save_map().tobytes() and merged != before
        assert m.remove_target_points(*sel, pose=pose) == out_a
        assert m.save_map().tobytes() == before
