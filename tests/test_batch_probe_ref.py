"""The one-point probes of tests/batch_probe_ref.py: the restated terms against the oracle, the placement caps, how many
probes are sharp, the measurement behind C_PROBE, and the proof that the probes bite - every mistake of
cell_record_ref.MUTANTS that a Sigma^-1 can show is caught by a named probe.  No GPU."""
import math

import numpy as np
import pytest

import batch_probe_ref as B
import cell_record_cases as K
import cell_record_ref as X

MODES = (0, 1)


def _all(dim):
    return K.catalogues(dim)


def _store32(rec):
    """The record as a device stores it: float32."""
    return {k: (v.astype(np.float32).astype(np.float64) if k in ("mean", "icov", "cov") else v) for k, v in rec.items()}


# ---------------------------------------------------------------------------------------------- the terms
@pytest.mark.parametrize("dim", [2, 3])
def test_restatement_equals_the_oracle(dim):
    """terms() against oracle.evaluate / evaluate3 (float64) on grids the oracle builds from the catalogue clouds, at
    the oracle's own records of the probe's cell: every entry to 1e-12 of its scale (the running-error scale A, which is
    the entry's size wherever nothing cancels)."""
    from oracle import ndt2d as o2, ndt3d as o3
    worst = 0.0
    for cat in _all(dim):
        sweep = B.sweep_cloud(cat)
        for p, (mp, er) in enumerate(K.PARAMS):
            if dim == 2:
                prm = [o2.NdtParams(cell_size=cat.c, min_points=mp, eig_ratio=er, hessian_mode=m) for m in MODES]
                grid = o2.build_grid(*cat.coords(sweep), prm[0])
                assert [grid.W, grid.H] == cat.ext
                ev = lambda pt, m: o2.evaluate(grid, pt[0:1], pt[1:2], (0.0, 0.0, 0.0), prm[m])
            else:
                prm = [o3.Ndt3Params(cell_size=cat.c, min_points=mp, eig_ratio=er, hessian_mode=m) for m in MODES]
                grid = o3.build_grid3(*cat.coords(sweep), prm[0])
                assert list(grid.dims) == cat.ext
                ev = lambda pt, m: o3.evaluate3(grid, pt[0:1], pt[1:2], pt[2:3], (0.0,) * 6, prm[m])
            pr = B.probes(cat, p)
            nv = pr["n_valid_probes"]
            keys = B.cell_key(pr["cell"][:nv], cat.ext)
            keep = np.flatnonzero(keys != (cat.big if cat.big is not None else -1))
            assert grid.valid[keys[keep]].all(), (cat.name, p)
            for m in MODES:
                out, A = B.terms(dim, pr["pt"][:nv], grid.mean[keys], grid.icov[keys], m)
                for j in keep:
                    H, g, sc, nh = ev(pr["pt"][j].astype(np.float64), m)
                    assert nh == 1
                    r = np.abs(B.row_vector(dim, H, g, sc) - out[j]) / np.where(A[j] > 0.0, A[j], 1.0)
                    assert r.max() <= 1e-12, (B.describe(cat, p, j), m, B.out_name(dim, int(np.argmax(r))), r.max())
                    worst = max(worst, float(r.max()))
            for j in range(nv, len(pr["pt"])):                       # the probes that must miss
                assert ev(pr["pt"][j].astype(np.float64), 0)[3] == 0, B.describe(cat, p, j)
    print(f"{dim}D: worst |terms - oracle| / A = {worst:.3g}")


# ---------------------------------------------------------------------------------------------- the placement
@pytest.mark.parametrize("dim", [2, 3])
def test_placement_caps_hold_for_every_catalogue_and_parameter_set(dim):
    lo, hi = math.inf, 0
    for cat in _all(dim):
        for p, (mp, er) in enumerate(K.PARAMS):
            pr = B.probes(cat, p)                                    # (asserts the caps itself)
            nv, exact = pr["n_valid_probes"], K.golden(cat, p)
            lo, hi = min(lo, nv), max(hi, nv)
            assert len(pr["unplaced"]) <= B.MAX_UNPLACED
            assert not pr["unplaced"] or (er == 1e-6 and cat.name.startswith("far")), (cat.name, p, pr["unplaced"])
            keys = B.cell_key(pr["cell"][:nv], cat.ext)
            assert pr["hit"][:nv].all() and not pr["hit"][nv:].any()
            assert set(keys.tolist()) == set(np.flatnonzero(exact["valid"]).tolist()), (cat.name, p)
            assert nv + len(pr["unplaced"]) == len(B.DIRECTIONS[dim]) * pr["n_valid_cells"] + pr["kind"].count("mean")
            # every probe lies where it is said to lie, by the kernels' own float32 rule
            origin = np.asarray(cat.h["origin"], dtype=np.float32)[0, :dim]
            f = np.floor((pr["pt"] - origin) * np.float32(1.0 / cat.c)).astype(np.int64)
            assert np.array_equal(f[:-1], pr["cell"][:-1]) and np.all(f[-1] == -3), (cat.name, p)
            miss = pr["kind"][nv:]
            n = cat.cells["n"].astype(np.int64)
            assert miss.count("invalid") == int(((n > 0) & ~exact["valid"]).sum())
            assert miss.count("corner") == 2 ** dim and miss.count("outside") == 1
            interior_empty = int((n == 0).sum()) - (int(np.prod(cat.ext)) - int(np.prod(np.array(cat.ext) - 2)))
            assert miss.count("empty") == (interior_empty if cat.name.startswith("lattice") else B.N_EMPTY_FAR)
    print(f"{dim}D: {lo} to {hi} probes of valid cells per (catalogue, parameter set)")
    assert (lo, hi) == ((39, 108) if dim == 2 else (60, 272))


@pytest.mark.parametrize("dim", [2, 3])
def test_at_least_half_of_the_lattice_probes_are_sharp(dim):
    """ulp32(probe) / sigma_min < 1e-3: the float32 grain of the probe's position is a thousandth of the cell's thinnest
    (clamped) extent, so the term reads the record and not the grain.  On the far catalogues, 700 m out (ulp32 = 6e-5 m), only
    the cells without a thin direction have such probes (printed, not asserted): what holds the batch there is the
    comparison with the single-pair path (tests/test_gpu_batch_records.py)."""
    def share(cat, p):
        pr, exact = B.probes(cat, p), K.golden(cat, p)
        nv = pr["n_valid_probes"]
        cov = exact["cov"][B.cell_key(pr["cell"][:nv], cat.ext)]
        S = np.zeros((nv, dim, dim))
        for q, (a, b) in enumerate(X.PAIRS[dim]):
            S[:, a, b] = S[:, b, a] = cov[:, q]
        sigma = np.sqrt(np.maximum(np.linalg.eigvalsh(S)[:, 0], 1e-300))
        return float(np.mean(X.ulp32(pr["pt"][:nv]).max(axis=1) / sigma < 1e-3))
    cats = _all(dim)
    for p in range(len(K.PARAMS)):
        s = share(cats[0], p)
        print(f"lattice{dim} {K.PARAMS[p]}: {100 * s:.0f} % sharp")
        assert s >= 0.5, (dim, p, s)
    far = [[share(c, p) for c in cats[1:]] for p in range(len(K.PARAMS))]
    print(f"far{dim}, share of sharp probes per parameter set (least to most over the catalogues): "
          + ", ".join(f"{K.PARAMS[p]}: {100 * min(v):.0f}-{100 * max(v):.0f} %" for p, v in enumerate(far)))


# ---------------------------------------------------------------------------------------------- C_PROBE
@pytest.mark.parametrize("dim", [2, 3])
def test_mirror_error_is_an_eighth_of_the_tolerance(dim):
    """The measurement behind C_PROBE: the oracle's float32 mirror on a one-cell grid holding the exact record rounded
    to float32, against terms() at that rounded record, every probe, both Hessian forms, in units of eps32 A."""
    worst = (0.0, None)
    for cat in _all(dim):
        for p in range(len(K.PARAMS)):
            pr, exact = B.probes(cat, p), K.golden(cat, p)
            nv = pr["n_valid_probes"]
            keys = B.cell_key(pr["cell"][:nv], cat.ext)
            mean32, icov32 = exact["mean"][keys].astype(np.float32), exact["icov"][keys].astype(np.float32)
            for m in MODES:
                out, A = B.terms(dim, pr["pt"][:nv], mean32, icov32, m)
                for j in range(nv):
                    got = B.mirror_terms(dim, pr["pt"][j], mean32[j], icov32[j], m)
                    err = np.abs(got - out[j])
                    assert not (err[A[j] == 0.0] > 0.0).any(), B.describe(cat, p, j)
                    u = err / np.where(A[j] > 0.0, B.EPS32 * A[j], 1.0)
                    if u.max() > worst[0]:
                        worst = (float(u.max()), (B.describe(cat, p, j), B.out_name(dim, int(np.argmax(u))), m))
    print(f"{dim}D: the mirror's worst error is {worst[0]:.3g} eps32 A at {worst[1]}")
    # float64 rounding, which differs between builds of numpy by a rounding or two: the documented figure within a factor 4
    assert B.MEASURED_UNITS[dim] / 4.0 <= worst[0] <= B.MEASURED_UNITS[dim] * 4.0, worst
    assert B.C_PROBE[dim] == math.ceil(8.0 * B.MEASURED_UNITS[dim]) and 8.0 * worst[0] <= B.C_PROBE[dim]


# ---------------------------------------------------------------------------------------------- the probes have teeth
def _as_a_device(cat, p, rec, mode):
    """(hit, rows) of the probes of (cat, p) read off the records `rec` by terms(): what a device with those records and
    exact arithmetic would put into its result rows."""
    pr = B.probes(cat, p)
    keys = np.concatenate([B.cell_key(pr["cell"][:-1], cat.ext), [0]])
    hit = rec["valid"][keys]
    hit[-1] = False
    rows = np.zeros((len(keys), B.nout(cat.dim)))
    rows[hit] = B.terms(cat.dim, pr["pt"][hit], rec["mean"][keys[hit]], rec["icov"][keys[hit]], mode)[0]
    return hit, rows


def _caught(cat, p, rec, mode):
    """[(probe, entry name, error / tolerance)] of the probes that tell `rec` from the exact records"""
    ref = B.reference(cat, p, mode)
    hit, rows = _as_a_device(cat, p, rec, mode)
    found = [(int(j), "hit", math.inf) for j in np.flatnonzero(hit != ref.hit)]
    r, e = ref.ratios(rows)
    for j in np.flatnonzero((hit == ref.hit) & (r > 1.0)):
        found.append((int(j), B.out_name(cat.dim, int(e[j])), float(r[j])))
    return found


@pytest.mark.parametrize("dim", [2, 3])
def test_correct_records_stored_as_float32_pass_every_probe(dim):
    """The control: the float64 restatement of the device formula, stored as float32, through exact arithmetic."""
    for cat in _all(dim):
        for p, (mp, er) in enumerate(K.PARAMS):
            rec = _store32(X.records_float64(cat.blob, mp, er))
            for m in MODES:
                found = _caught(cat, p, rec, m)
                assert not found, [(B.describe(cat, p, j), e, r) for j, e, r in found[:3]]


# (mutant, dim) -> (catalogue, index into PARAMS, the cell's case, the probe's direction and step, Hessian form) that must
# catch it.  All on the lattice catalogues.
CAUGHT_BY = {
    ("divide_by_n", 2): ("lattice2", 1, "random3", "dir1 s=1", 1),
    ("divide_by_n", 3): ("lattice3", 4, "clamp_mid_1e-06_above", "dir0 s=1", 1),
    ("clamp_at_second", 2): ("lattice2", 0, "rect_wide", "dir0 s=1", 0),
    ("clamp_at_second", 3): ("lattice3", 0, "rect_wide", "dir0 s=1", 0),
    ("clamp_at_trace", 2): ("lattice2", 4, "clamp_1_below", "dir1 s=1", 1),
    ("clamp_at_trace", 3): ("lattice3", 4, "cell_corners", "dir0 s=0.5", 0),
    ("float32_reciprocal", 2): ("lattice2", 0, "clamp_1_below", "dir0 s=1", 0),
    ("float32_reciprocal", 3): ("lattice3", 0, "rot_cube", "dir1 s=1", 0),
    ("float64_numerator", 2): ("lattice2", 0, "far_tight64", "dir0 s=1", 0),
    ("float64_numerator", 3): ("lattice3", 0, "far_tight64", "dir2 s=1", 0),
}
# Mistakes no probe catches, whatever its direction.  three_sweeps in 3D: three Jacobi sweeps leave Sigma^-1 within its
# storage tolerance on every lattice cell and at most 8 such tolerances (5e-7 of the norm) off on a few cells of the far
# catalogues - below the float32 rounding of a single per-point term (the arithmetic part, about ten roundings), so an
# evaluation cannot show it; reading the record back can (test_cell_record_ref.CAUGHT_BY: the clamped Sigma of a far
# cell).  The others change no record at all: 2D has no sweeps, 3D no half_df, and half_df_gt is no mutant
# (test_cell_record_ref.test_half_df_gt_is_no_mutant).
OUT_OF_REACH = (("three_sweeps", 3),)
NO_CHANGE = (("three_sweeps", 2), ("half_df_gt", 2), ("half_df_gt", 3))


def test_every_mutant_is_accounted_for():
    assert sorted(list(CAUGHT_BY) + list(OUT_OF_REACH) + list(NO_CHANGE)) == sorted((m, d) for m in X.MUTANTS for d in (2, 3))


@pytest.mark.parametrize("mutant,dim", sorted(CAUGHT_BY))
def test_mutant_is_caught_by_a_named_probe(mutant, dim):
    name, p, case, kind, mode = CAUGHT_BY[(mutant, dim)]
    cat = B.catalogue(name)
    assert name.startswith("lattice")
    mp, er = K.PARAMS[p]
    found = _caught(cat, p, _store32(X.records_float64(cat.blob, mp, er, mutant=mutant)), mode)
    pr = B.probes(cat, p)
    named = [(j, e, r) for j, e, r in found
             if pr["kind"][j] == kind and cat.cell_name(B.cell_key(pr["cell"][j][None], cat.ext)[0]) == case]
    print(mutant, dim, "caught by", [(B.describe(cat, p, j), e, r) for j, e, r in named], "and", len(found) - len(named), "more")
    assert named, (mutant, dim, [(B.describe(cat, p, j), e, r) for j, e, r in found[:5]])


@pytest.mark.parametrize("mutant,dim", OUT_OF_REACH + NO_CHANGE)
def test_mutant_no_probe_can_catch(mutant, dim):
    for cat in _all(dim):
        for p, (mp, er) in enumerate(K.PARAMS):
            rec = X.records_float64(cat.blob, mp, er, mutant=mutant)
            if (mutant, dim) in NO_CHANGE:
                plain = X.records_float64(cat.blob, mp, er)
                assert all(np.array_equal(rec[f], plain[f]) for f in ("valid", "mean", "icov")), (cat.name, p)
                continue
            exact = K.golden(cat, p)
            k = np.flatnonzero(exact["valid"])
            assert np.array_equal(rec["valid"], exact["valid"])
            got = _store32(rec)
            within = np.abs(got["icov"][k] - exact["icov"][k]) / X.matrix_tolerance(exact["icov"][k], exact["kappa"][k])
            assert within.max() <= (1.0 if cat.name.startswith("lattice") else 8.0), (cat.name, p, within.max())
            assert np.all(np.abs(got["mean"][k] - exact["mean"][k]) <= X.mean_tolerance(exact["mean"][k], X.all_centres(cat.h)[k], cat.c))
            for m in MODES:
                assert not _caught(cat, p, got, m), (cat.name, p, m)
