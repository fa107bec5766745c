"""The grid build inside the batch kernels (process_pair of csrc/ndt2d_batch.hpp, process_pair3 of csrc/ndt3d_batch.hpp:
bounding box and geometry, per-cell counts, compaction into slots, exact sums, finalise), held cell by cell to the exact
records of tests/golden/cell_records.npz - the records tests/test_gpu_cell_records.py holds every other build to.

The batch has no read-back of its records.  What it has: with fixed_iterations = 1 a result row holds H, g, score and n_hit
of the evaluation at the start pose.  A pair whose source is one point inside one chosen cell, at the identity pose, reads
that cell's valid bit exactly and its mean and Sigma^-1 through a single term (tests/batch_probe_ref.py: the probes, the
float64 terms, the tolerance).  A catalogue is that many tiny pairs in one batch call: the target is the catalogue's cloud
once per probe, the source the probe.

Variants, each forced and checked to have run: 2D small (last_large_count == 0), 2D 1024 threads (== n_pairs), 2D global
tables (one more target point far beyond the maximum corner: more than 20480 cells, the catalogue's cells where they
were), 2D global tables with overlap_grids = 4 (c = 0.3 catalogues; against the float64 restatement of the four-grid blob a
single-pair handle saves, at twice the constant; n_hit = the grids whose cell at the probe is valid), 3D on chip, 3D
global tables (stretched the same way over the on-chip voxels).  Each variant runs three of the five parameter sets,
rotating, and both Hessian forms on the lattice catalogues.

Per probe:  a. n_hit is the exact valid bit; a miss has exact zeros and NDT_TOO_FEW_HITS, a hit one of OK / NOT_CONVERGED /
DEGENERATE_HESSIAN;  b. every entry of H, g, score within batch_probe_ref's tolerance of the exact-record reference;
c. 2D, one grid: the row equals (==) NdtMatcher2D.evaluate of the same point on a handle whose set_target got the same
cloud - the header's "bit-identical records" claim, and what holds the catalogues 700 m out, where (b) is wide;
d. 3D: the same against NdtMatcher3D.evaluate within twice the arithmetic part (the batch sums in the map frame);
e. the variants of one dimension give equal rows on every (catalogue, parameter set, Hessian form) they share.

The 2^20-point cell: the sweeps above run on the cloud without that cell's points (batch_probe_ref.sweep_cloud); the full
cloud, 1.05 M points, runs as four pairs - three probes in the full cell, one in another - on the 1024-thread and global
variants in 2D (the small variant must hand the pairs over) and on both 3D variants: 32-bit counters, 64-bit atomics.
One point more in that cell (2^20 + 1): ndt*_set_target answers NDT_ERR_CAPACITY, the batch makes the cell invalid and
aligns on the rest (include/ndt_hip.h) - the full cell's probes miss, the other probe's row is what it was.

Worst error / tolerance of (b) per variant, as measured on an MI355X (WORST_MEASURED; a run prints the current one, a
failure message too): 2D small 0.213, 1024 threads 0.236, global tables 0.236, 3D on chip 0.405, global tables 0.405, the
full cloud 0.158 (2D) and 0.318 (3D), four overlapping grids 0.200.  (c) held as equality on every 2D probe."""
import itertools

import numpy as np
import pytest

import batch_probe_ref as B
import cell_record_cases as K
import cell_record_ref as X
import step_replay as SR

pytestmark = pytest.mark.gpu

# variant -> worst |device - reference| / tolerance of assertion (b) over its sweeps, measured on an MI355X
WORST_MEASURED = {"2d-small": 0.213, "2d-1024": 0.236, "2d-global": 0.236, "3d-onchip": 0.405, "3d-global": 0.405,
                  "2d-global-overlap4": 0.200}

NDT_OK, NDT_NOT_CONVERGED, NDT_DEGENERATE_HESSIAN, NDT_TOO_FEW_HITS = 0, 1, 2, 3
HIT_STATUS = (NDT_OK, NDT_NOT_CONVERGED, NDT_DEGENERATE_HESSIAN)

# name -> (dim, constructor options, stretched past this many cells or None, last_large_count as a share of the pairs)
VARIANTS = {
    "2d-small": (2, dict(small_variant=True), None, 0),
    "2d-1024": (2, dict(small_variant=False), None, 1),
    "2d-global": (2, dict(global_workgroups=8), SR.GLOBAL2D_ONCHIP_CELLS, 1),
    "3d-onchip": (3, dict(), None, None),
    "3d-global": (3, dict(global_workgroups=8), SR.GLOBAL3D_ONCHIP_CELLS, None),
}
ORDER = {2: ["2d-small", "2d-1024", "2d-global"], 3: ["3d-onchip", "3d-global"]}

_rows_seen = {}       # (catalogue, parameter set, mode) -> (variant, rows) of the first variant that ran it
_single_seen = {}     # (catalogue, parameter set, mode, stretched) -> rows of the single-pair handle's evaluate


def _api(dim):
    from gtsam_ndt_amd import matcher as M
    return (M.NdtMatcher2D, M.NdtBatch2D) if dim == 2 else (M.NdtMatcher3D, M.NdtBatch3D)


def _options(cat, p, mode, **more):
    mp, er = K.PARAMS[p]
    return dict(cell_size=cat.c, min_points=mp, eig_ratio=er, hessian_mode=mode, fixed_iterations=1, min_hits=1, **more)


def _rows(dim, results):
    """[n, nout + 2]: H, g, score in batch_probe_ref's layout, n_hit, status"""
    return np.array([np.concatenate([B.row_vector(dim, r.H, r.g, r.score), [r.n_hit, r.status]]) for r in results])


def _batch_rows(variant, cat, p, mode, cloud, pts, more=None):
    dim, how, _, large = VARIANTS[variant]
    _, Batch = _api(dim)
    target = cat.coords(cloud)
    zero = (0.0,) * B.NPOSE[dim]
    with Batch(**how, **_options(cat, p, mode, **(more or {}))) as b:
        res = b.align([target] * len(pts), [tuple(pt[a:a + 1] for a in range(dim)) for pt in pts], [zero] * len(pts))
        if large is not None:
            assert b.last_large_count == large * len(pts), (variant, cat.name, b.last_large_count, len(pts))
    return _rows(dim, res)


def _single_rows(dim, cat, p, mode, cloud, pts, key):
    if key not in _single_seen:
        Matcher, _ = _api(dim)
        mp, er = K.PARAMS[p]
        zero = (0.0,) * B.NPOSE[dim]
        with Matcher(cell_size=cat.c, min_points=mp, eig_ratio=er, hessian_mode=mode) as m:
            m.set_target(*cat.coords(cloud))
            out = []
            for pt in pts:
                H, g, score, n_hit = m.evaluate(*[pt[a:a + 1] for a in range(dim)], zero)
                out.append(np.concatenate([B.row_vector(dim, H, g, score), [n_hit]]))
        _single_seen[key] = np.array(out)
    return _single_seen[key]


def _check_rows(what, dim, rows, ref, names, worst):
    """assertions a and b on the rows of one batch call against a batch_probe_ref.Reference; keeps the worst ratio"""
    n_out = B.nout(dim)
    hit = ref.hit.astype(bool)
    n_hit, status = rows[:, n_out].astype(int), rows[:, n_out + 1].astype(int)
    bad = np.flatnonzero(n_hit != hit.astype(int))
    assert bad.size == 0, (what, "n_hit is not the exact valid bit", [(names(j), int(n_hit[j])) for j in bad[:5]])
    assert not rows[~hit, :n_out].any(), (what, "a miss with a term", [names(j) for j in np.flatnonzero(~hit)[:5]])
    assert np.all(status[~hit] == NDT_TOO_FEW_HITS), (what, status[~hit])
    assert np.all(np.isin(status[hit], HIT_STATUS)), (what, status[hit])
    r, (j, e) = ref.worst(rows[:, :n_out])
    if r >= worst[0]:
        worst[:] = [r, f"{names(j)} {B.out_name(dim, e)}"]
    assert r <= 1.0, (f"{what}: {B.out_name(dim, e)} of {names(j)} is {rows[j, e]!r}, reference {ref.out[j, e]!r}: {r:.3g} times "
                      f"the tolerance {ref.tol[j, e]:.3g} (worst so far {worst})")


def _targets(variant, cat, cloud):
    dim, _, over, _ = VARIANTS[variant]
    if over is None:
        assert int(np.prod(cat.ext)) <= over_limit(dim)
        return cloud, False
    more, k, ext = B.stretched(cat, cloud, over)
    assert int(np.prod(ext)) > over and max(ext) < 512
    return more, True


def over_limit(dim):
    return SR.GLOBAL2D_ONCHIP_CELLS if dim == 2 else SR.GLOBAL3D_ONCHIP_CELLS


def _compare_with_single(what, dim, rows, single, arith, names):
    """assertions c (2D: equality) and d (3D: twice the arithmetic part)"""
    n_out = B.nout(dim)
    assert np.array_equal(rows[:, n_out], single[:, n_out]), (what, "n_hit differs from the single-pair path")
    if dim == 2:
        bad = np.flatnonzero((rows[:, :n_out] != single[:, :n_out]).any(axis=1))
        assert bad.size == 0, (what, "not the single-pair path's terms to the bit", [
            (names(j), (rows[j, :n_out] - single[j, :n_out]).tolist()) for j in bad[:3]])
    else:
        r, (j, e) = B.Reference(None, single[:, :n_out], 2.0 * arith, arith, {}).worst(rows[:, :n_out])
        assert r <= 1.0, (what, f"{B.out_name(dim, e)} of {names(j)}: {rows[j, e]!r} against the single-pair path's "
                          f"{single[j, e]!r}, {r:.3g} times twice the arithmetic part")


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_batch_grid_build_against_the_exact_records(gpu_lib, variant):
    dim = VARIANTS[variant][0]
    j = ORDER[dim].index(variant)
    worst = [0.0, ""]
    for cat in K.catalogues(dim):
        cloud, stretched = _targets(variant, cat, B.sweep_cloud(cat))
        for p in sorted((j + t) % len(K.PARAMS) for t in range(3)):
            pr = B.probes(cat, p)
            keep = np.ones(len(pr["pt"]), bool)
            if cat.big is not None:                                  # the 2^20-point cell is empty in the sweep cloud
                keep[:-1] = B.cell_key(pr["cell"][:-1], cat.ext) != cat.big
            sel = np.flatnonzero(keep)
            names = lambda k: B.describe(cat, p, int(sel[k]))
            for mode in ((0, 1) if cat.big is not None else (0,)):
                what = f"{variant} {cat.name} {K.PARAMS[p]} hessian_mode {mode}"
                ref = B.reference(cat, p, mode).select(sel)
                rows = _batch_rows(variant, cat, p, mode, cloud, pr["pt"][sel])
                _check_rows(what, dim, rows, ref, names, worst)
                single = _single_rows(dim, cat, p, mode, cloud, pr["pt"][sel], (cat.name, p, mode, stretched))
                _compare_with_single(what, dim, rows, single, ref.arith_bound(), names)
                first = _rows_seen.setdefault((cat.name, p, mode), (variant, rows))
                assert np.array_equal(first[1], rows), f"{what}: rows differ from variant {first[0]}"
    print(f"worst error / tolerance, {variant}: {worst[0]:.3g} at {worst[1]} (measured before: {WORST_MEASURED.get(variant)})")


def test_overlapping_grids_against_the_float64_restatement(gpu_lib):
    """overlap_grids = 4 on the c = 0.3 catalogues: the probe scores against the cell it lies in of each of the four grids
    (the kernels' float32 rule); the records are the float64 restatement of the four-grid blob a single-pair handle with
    the same option saves, held at twice the constant."""
    import map_coarsen_ref as R
    from gtsam_ndt_amd.matcher import NdtBatch2D, NdtMatcher2D
    worst = [0.0, ""]
    for cat in K.catalogues(2)[1:]:
        for p in (0, 2, 3):
            mp, er = K.PARAMS[p]
            what = f"2d-global overlap_grids=4 {cat.name} {K.PARAMS[p]}"
            with NdtMatcher2D(cell_size=cat.c, min_points=mp, eig_ratio=er, overlap_grids=4) as m:
                m.set_target(*cat.coords())
                blob = m.save_map()
            h, cells = R.parse(blob)
            assert h["ngrid"] == 4
            rec = X.records_float64(blob, mp, er)
            ext, ncell = [h["width"], h["height"]], h["width"] * h["height"]
            pts = B.probes(cat, p)["pt"]
            names = lambda k: B.describe(cat, p, int(k))
            # per probe and grid the admissible (out, tol) of the grid's cell at the probe: one, or several where the
            # cell's mean lies on a float32 rounding tie; the row has to meet the sum of one choice per grid
            choices = [[] for _ in pts]
            n_hit = np.zeros(len(pts), int)
            ctr = X.all_centres(h)
            for q in range(4):
                origin = np.asarray(h["origin"], dtype=np.float32)[q, :2]
                f = np.floor((pts - origin) * np.float32(1.0 / cat.c)).astype(np.int64)
                inside = np.all((f >= 0) & (f < np.array(ext)), axis=1)
                keys = q * ncell + B.cell_key(np.where(inside[:, None], f, 0), ext)
                on = np.flatnonzero(inside & rec["valid"][keys])
                if on.size == 0:
                    continue
                o, t, ar, alt = B.tolerance(2, pts[on], rec, keys[on], ctr[keys[on]], cat.c, 0, c_record=2 * X.C_RECORD)
                for j, k in enumerate(on):
                    choices[k].append([(o[j], t[j])] + [(oo, tt) for oo, tt, _ in alt.get(j, [])])
                n_hit[on] += 1
            with NdtBatch2D(global_workgroups=8, **_options(cat, p, 0, overlap_grids=4)) as b:
                zero = (0.0, 0.0, 0.0)
                res = b.align([cat.coords()] * len(pts), [(pt[0:1], pt[1:2]) for pt in pts], [zero] * len(pts))
            rows = _rows(2, res)
            got_hit = rows[:, B.nout(2)].astype(int)
            assert np.array_equal(got_hit, n_hit), (what, [(names(k), int(got_hit[k]), int(n_hit[k])) for k in np.flatnonzero(got_hit != n_hit)[:5]])
            assert not rows[n_hit == 0, :B.nout(2)].any() and np.all(rows[n_hit == 0, -1] == NDT_TOO_FEW_HITS), what
            assert np.all(np.isin(rows[n_hit > 0, -1], HIT_STATUS)), what
            for k in range(len(pts)):
                best = (np.inf, 0, None)
                for pick in itertools.product(*choices[k]):
                    out, tol = sum(o for o, _ in pick) + np.zeros(B.nout(2)), sum(t for _, t in pick) + np.zeros(B.nout(2))
                    r, (_, e) = B.Reference(None, out[None], tol[None], tol[None], {}).worst(rows[k:k + 1, :B.nout(2)])
                    if r < best[0]:
                        best = (r, e, out)
                r, e, out = best
                if r >= worst[0]:
                    worst[:] = [r, f"{names(k)} {B.out_name(2, e)}"]
                assert r <= 1.0, f"{what}: {B.out_name(2, e)} of {names(k)} is {rows[k, e]!r}, reference {out[e]!r}: {r:.3g} times the tolerance"
            assert n_hit.max() >= 2 and (n_hit == 0).any(), what
    print(f"worst error / tolerance, 2d-global overlap_grids=4: {worst[0]:.3g} at {worst[1]} "
          f"(measured before: {WORST_MEASURED.get('2d-global-overlap4')})")


# ---------------------------------------------------------------------------------------------- the 2^20-point cell
def _big_probes(cat, p):
    """indices into probes(cat, p): three probes of the 2^20-point cell and one of another valid cell"""
    pr = B.probes(cat, p)
    nv = pr["n_valid_probes"]
    in_big = B.cell_key(pr["cell"][:nv], cat.ext) == cat.big
    sel = np.concatenate([np.flatnonzero(in_big)[:3], np.flatnonzero(~in_big)[:1]])
    assert len(sel) == 4
    return sel


BIG = {"2d-1024": dict(small_variant=True), "2d-global": dict(global_workgroups=8), "3d-onchip": dict(), "3d-global": dict(global_workgroups=8)}


@pytest.mark.parametrize("variant", list(BIG))
def test_the_full_cell_of_2_to_the_20_points(gpu_lib, variant):
    """The lattice catalogue's full cloud, four pairs.  2D: the small variant runs first and must hand every pair over."""
    dim, _, over, _ = VARIANTS[variant]
    cat = K.catalogues(dim)[0]
    _, Batch = _api(dim)
    p, mode = 0, 0
    assert cat.cells["n"][cat.big] == 1 << 20
    cloud = cat.cloud if over is None else B.stretched(cat, cat.cloud, over)[0]
    sel = _big_probes(cat, p)
    pts = B.probes(cat, p)["pt"][sel]
    names = lambda k: B.describe(cat, p, int(sel[k]))
    what = f"{variant} {cat.name}, the full cloud, {K.PARAMS[p]}"
    ref = B.reference(cat, p, mode).select(sel)
    zero = (0.0,) * B.NPOSE[dim]
    with Batch(**BIG[variant], **_options(cat, p, mode)) as b:
        res = b.align([cat.coords(cloud)] * 4, [tuple(pt[a:a + 1] for a in range(dim)) for pt in pts], [zero] * 4)
        if dim == 2:
            assert b.last_large_count == 4, (what, b.last_large_count)
    rows = _rows(dim, res)
    worst = [0.0, ""]
    _check_rows(what, dim, rows, ref, names, worst)
    single = _single_rows(dim, cat, p, mode, cloud, pts, (cat.name, p, mode, over is not None, "full"))
    _compare_with_single(what, dim, rows, single, ref.arith_bound(), names)
    first = _rows_seen.setdefault((cat.name, p, mode, "full"), (variant, rows))
    assert np.array_equal(first[1], rows), f"{what}: rows differ from variant {first[0]}"
    print(f"worst error / tolerance, {what}: {worst[0]:.3g} at {worst[1]}")


@pytest.mark.parametrize("variant", ["2d-1024", "3d-onchip"])
def test_one_point_too_many_makes_the_cell_invalid(gpu_lib, variant):
    """2^20 + 1 points in a cell: ndt*_set_target answers NDT_ERR_CAPACITY; the batch kernels' n <= 2^20 test makes the cell
    invalid and aligns on the rest (the batch comment of include/ndt_hip.h)."""
    from gtsam_ndt_amd import _lib as L
    dim = VARIANTS[variant][0]
    cat = K.catalogues(dim)[0]
    Matcher, Batch = _api(dim)
    p, mode = 0, 0
    sel = _big_probes(cat, p)
    pts = B.probes(cat, p)["pt"][sel]
    centre = X.centres(cat.h, [cat.big])[0].astype(np.float32)
    assert np.array_equal(centre.astype(np.float64), X.centres(cat.h, [cat.big])[0])
    more = np.concatenate([cat.cloud, centre[None]])
    zero = (0.0,) * B.NPOSE[dim]
    sources = [tuple(pt[a:a + 1] for a in range(dim)) for pt in pts]
    with Batch(**BIG[variant], **_options(cat, p, mode)) as b:
        full = _rows(dim, b.align([cat.coords()] * 4, sources, [zero] * 4))
        over = _rows(dim, b.align([cat.coords(more)] * 4, sources, [zero] * 4))
    n_out = B.nout(dim)
    assert np.all(full[:, n_out] == 1), full[:, n_out]
    assert not over[:3, :n_out + 1].any() and np.all(over[:3, -1] == NDT_TOO_FEW_HITS), over[:3]
    assert np.array_equal(over[3], full[3]), (over[3], full[3])
    mp, er = K.PARAMS[p]
    with Matcher(cell_size=cat.c, min_points=mp, eig_ratio=er) as m:
        with pytest.raises(L.NdtError) as err:
            m.set_target(*cat.coords(more))
        assert err.value.code == L.NDT_ERR_CAPACITY, err.value
