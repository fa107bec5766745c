"""Every device path that forms per-cell records, on the catalogue of tests/cell_record_cases.py (degenerate, clamped,
ill-conditioned, full and far-away cells), against the exact records committed in tests/golden/cell_records.npz.

For each path, catalogue and (min_points, eig_ratio):
  1. save_map() is the catalogue's blob byte for byte - the sums are the known ones;
  2. grid() has the exact valid mask, grid_info().n_valid its count;
  3. means and Sigma^-1 are within  ulp32 / 2 + C_RECORD eps64 kappa N  of the exact values (tests/cell_record_ref.py:
     the tolerance, and the measurement behind C_RECORD);
  4. components() lists the valid cells in key order with their means, and Sigma within the same tolerance
     (k_cov_records / k_cov_records3);
and all paths of one catalogue and parameter set give bit-identical grid() and components() arrays.

Paths: load_map of the forged blob (k_finalise<1> / k_finalise3<1> via ndt_map_io.hpp); 2D set_target with binned_build
0, 1, 2 (k_finalise, k_tile_gather, the round-1 binned build) and single_sync_build 0 and 1, 3D set_target
(k_tile_accumulate3) with single_sync_build 0 and 1; set_target of one half of the cloud + add_target_points of the other;
the cloud plus a seeded extra cloud, then remove_target_points of the extra (k_finalise<-1> / k_finalise3<-1> and the
signed tile kernels); overlap_grids = 4 in 2D on the c = 0.3 catalogues, where the four shifted grids have no committed
expectation and the float64 restatement of the handle's own save_map stands in at twice the constant.

Each path runs three of the five parameter sets, rotating, so every set meets several paths.

The grid build inside k_batch / k_batch3 has no read-back of its records: tests/test_gpu_batch_records.py holds it to the
same exact records through one-point probes of every cell of these catalogues (tests/batch_probe_ref.py)."""
import numpy as np
import pytest

import cell_record_cases as K
import cell_record_ref as X

pytestmark = pytest.mark.gpu

_seen = {}          # (catalogue, parameter set) -> (path, grid() and components() arrays) of the first path that ran


def _matcher(dim, cat, p, tuning=None, **kw):
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D
    mp, er = K.PARAMS[p]
    return (NdtMatcher2D if dim == 2 else NdtMatcher3D)(cell_size=cat.c, min_points=mp, eig_ratio=er, tuning=tuning, **kw)


def _check(m, cat, p, path, worst):
    exact = K.golden(cat, p)
    what = f"{path} {cat.name} {K.PARAMS[p]}"
    assert np.array_equal(m.save_map(), cat.blob), what
    count, mean, icov = m.grid()
    assert np.array_equal(count.astype(np.int64), cat.cells["n"].astype(np.int64)), what
    got_valid = icov[:, 0] != 0
    bad = np.flatnonzero(got_valid != exact["valid"])
    assert bad.size == 0, (what, [cat.cell_name(k) for k in bad[:5]])
    assert m.grid_info().n_valid == int(exact["valid"].sum()), what
    w = X.check_records(dict(mean=mean, icov=icov), exact, cat.h, what=what, name=cat.cell_name)
    key, cmean, ccov = m.components()
    assert np.array_equal(key, np.flatnonzero(exact["valid"]).astype(np.int32)), what
    assert np.array_equal(cmean, mean[key]), what
    cov = np.zeros_like(icov)
    cov[key] = ccov
    w.update(X.check_records(dict(cov=cov), exact, cat.h, what=what, name=cat.cell_name))
    for f, (u, k) in w.items():
        if u >= worst.get(f, (-1.0,))[0]:
            worst[f] = (u, cat.name, K.PARAMS[p], cat.cell_name(k))
    arrays = (count, mean, icov, key, cmean, ccov)
    first = _seen.setdefault((cat.name, p), (path, arrays))
    for a, b in zip(first[1], arrays):
        assert np.array_equal(a, b), f"{what}: not bit-identical to path {first[0]}"


def _load_map(dim, cat, p):
    m = _matcher(dim, cat, p)
    m.load_map(cat.blob)
    return m


def _set_target(tuning, twice=False):
    def run(dim, cat, p):
        m = _matcher(dim, cat, p, tuning=tuning)
        m.set_target(*cat.coords())
        if twice:                                   # the single-sync build needs the storage of an earlier build
            m.set_target(*cat.coords())
        return m
    return run


def _half_then_add(dim, cat, p):
    first = np.zeros(len(cat.cloud), bool)
    first[::2] = True
    first[cat.extent_points()] = True               # the half that is set first spans the whole cloud's grid
    m = _matcher(dim, cat, p)
    m.set_target(*cat.coords(cat.cloud[first]))
    assert m.add_target_points(*cat.coords(cat.cloud[~first])) == 0
    return m


def _add_then_remove(dim, cat, p):
    extra = K.extra_cloud(cat, 2000 if cat.big is not None else 150)
    m = _matcher(dim, cat, p)
    m.set_target(*cat.coords(np.concatenate([cat.cloud[::3], extra, cat.cloud[1::3], cat.cloud[2::3]])))
    assert m.remove_target_points(*cat.coords(extra)) == 0
    return m


PATHS2 = [("load_map", _load_map), ("binned_build=0", _set_target({"binned_build": 0})),
          ("binned_build=1", _set_target({"binned_build": 1})), ("binned_build=2", _set_target({"binned_build": 2})),
          ("single_sync_build=0", _set_target({"single_sync_build": 0}, twice=True)),
          ("single_sync_build=1", _set_target({"single_sync_build": 1}, twice=True)),
          ("half_then_add", _half_then_add), ("add_then_remove", _add_then_remove)]
PATHS3 = [("load_map", _load_map), ("single_sync_build=0", _set_target({"single_sync_build": 0}, twice=True)),
          ("single_sync_build=1", _set_target({"single_sync_build": 1}, twice=True)),
          ("half_then_add", _half_then_add), ("add_then_remove", _add_then_remove)]


@pytest.mark.parametrize("dim,j", [(2, j) for j in range(len(PATHS2))] + [(3, j) for j in range(len(PATHS3))],
                         ids=[f"2d-{n}" for n, _ in PATHS2] + [f"3d-{n}" for n, _ in PATHS3])
def test_records_of_every_path_against_the_exact_reference(gpu_lib, dim, j):
    path, build = (PATHS2 if dim == 2 else PATHS3)[j]
    worst = {}
    for cat in K.catalogues(dim):
        for p in sorted((j + t) % len(K.PARAMS) for t in range(3)):
            with build(dim, cat, p) as m:
                _check(m, cat, p, f"{dim}D {path}", worst)
    print(f"worst device error, {dim}D {path}, in units of eps64 kappa N beyond the float32 store "
          f"(C_RECORD = {X.C_RECORD:g}): {worst}")


def test_overlapping_grids_against_the_float64_restatement(gpu_lib):
    """overlap_grids = 4 on the c = 0.3 catalogues: grid 0 of the four (what grid() hands out) against records_float64 of
    the handle's own save_map at 2 C_RECORD, the valid count over all four grids.  (No covariance records here:
    map-to-map alignment, and with it components(), does not take overlapping grids.)"""
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    import map_coarsen_ref as R
    worst = {}
    for cat in K.catalogues(2)[1:]:
        for p in (0, 2, 3):
            mp, er = K.PARAMS[p]
            what = f"overlap {cat.name} {K.PARAMS[p]}"
            with NdtMatcher2D(cell_size=cat.c, min_points=mp, eig_ratio=er, overlap_grids=4) as m:
                m.set_target(*cat.coords())
                blob = m.save_map()
                h, cells = R.parse(blob)
                assert h["ngrid"] == 4 and int(cells["n"].sum()) == 4 * len(cat.cloud), what
                ref = X.records_float64(blob, mp, er)
                ncell = h["width"] * h["height"]
                count, mean, icov = m.grid()
                assert np.array_equal(count.astype(np.int64), cells["n"][:ncell].astype(np.int64)), what
                assert np.array_equal(icov[:, 0] != 0, ref["valid"][:ncell]), what
                assert m.grid_info().n_valid == int(ref["valid"].sum()), what
                w = X.check_records(dict(mean=mean, icov=icov), ref, h, c=2 * X.C_RECORD, what=what)
                for f, (u, k) in w.items():
                    if u >= worst.get(f, (-1.0,))[0]:
                        worst[f] = (u, cat.name, K.PARAMS[p], int(k))
    print(f"worst device error against records_float64, overlap_grids = 4: {worst}")
