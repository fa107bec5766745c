"""The target-side lattice rule (gtsam_ndt_amd/csrc/ndt_lattice.hpp: the grid of a cloud, the cell of a target point, the
terms a point adds to its cell's exact sums) on the CPU: the functions every build kernel and the host geometry call, in
a stand-alone program under gcc's AddressSanitizer and UndefinedBehaviorSanitizer, held to integer equality with the
Python statements of the rule (tests/map_coarsen_ref.py, tests/seam_ref.py, tests/cell_record_ref.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import cell_record_cases as CC
import map_coarsen_ref as R
import seam_cases as SC
import seam_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
RING = {2: 1, 3: 0}                      # kRing2, kRing3
MUTANTS = ("divide", "truncate", "upper_inclusive")
TERM_CLOUDS = [(2, 0.3, 0.0), (3, 0.3, 0.0), (2, 0.1, 5.0), (2, 0.5, 700.0), (3, 0.7, -650.0)]      # (dim, c, centre)
N_TERM_POINTS = 20000


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("san") / "lattice")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gtsam_ndt_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "lattice_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


def _run(driver, lines):
    p = subprocess.run([driver], input="".join(lines), capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    out = p.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def _bits(v):
    return int(np.array(v, F32).view(np.uint32))


def _geometry_line(dim, c, lo, hi):
    return f"G {dim} {float(c)!r} " + " ".join(f"{_bits(lo[a])} {_bits(hi[a])}" for a in range(dim)) + "\n"


def _point_line(dim, c, origin, ext, p):
    return f"P {dim} {float(c)!r} " + " ".join(f"{_bits(origin[a])} {int(ext[a])} {_bits(p[a])}" for a in range(dim)) + "\n"


def _seam_targets():
    return [SC.target(dim, c, base) for dim, tt in ((2, SC.TARGETS_2D), (3, SC.TARGETS_3D)) for c, base in tt]


# ------------------------------------------------------------------------------------------------ geometry
def test_geometry_equals_the_references(driver):
    lines, want = [], []
    for dim in (2, 3):
        for cat in CC.catalogues(dim):
            origin, ext = R.grid_geometry(cat.cloud, cat.c)
            lines.append(_geometry_line(dim, cat.c, cat.cloud.min(axis=0), cat.cloud.max(axis=0)))
            want.append((cat.name, origin, ext))
    for t in _seam_targets():
        P = np.stack(t.coords, axis=1)
        origin, ext = R.grid_geometry(P, t.c)
        assert [_bits(v) for v in origin] == [_bits(v) for v in t.origin] and list(ext) == list(t.ext), t.name
        assert _bits(t.grid.inv_c) == _bits(F32(1.0 / t.c)), t.name
        lines.append(_geometry_line(t.dim, t.c, P.min(axis=0), P.max(axis=0)))
        want.append((t.name, t.origin, t.ext))
    assert len(lines) >= 10 + len(SC.TARGETS_2D) + len(SC.TARGETS_3D)
    for (name, origin, ext), line in zip(want, _run(driver, lines)):
        assert line == "ok " + " ".join(f"{_bits(o)} {int(e)}" for o, e in zip(origin, ext)), (name, line)


def test_what_is_no_grid_is_reported_and_not_undefined(driver):
    inf, big = np.inf, np.finfo(np.float32).max
    cases = [
        (2, 0.3, (inf, inf), (-inf, -inf), "none"),                    # what the bounds reduction leaves of a cloud of NaNs
        (3, 0.5, (0.0, inf, 0.0), (1.0, -inf, 1.0), "none"),
        (2, 0.3, (np.nan, 0.0), (np.nan, 1.0), "none"),
        (2, 0.3, (-big, 0.0), (big, 1.0), "capacity"),                 # k is infinite: max - origin overflows float32
        (2, 0.3, (0.0, -inf), (1.0, inf), "capacity"),                 # k is not a number: inf - inf
        (3, 1.0, (0.0, 0.0, -1e30), (1.0, 1.0, 1e30), "capacity"),     # k = 2e30, far beyond any int
        (2, 1e-8, (0.0, 0.0), (1.0, 1.0), "capacity"),                 # k = 1e8 > 1e7 per axis
        (2, 1e-4, (0.0, 0.0), (2.0, 2.0), "capacity"),                 # 20 002^2 > 2^27 cells
        (3, 0.01, (0.0, 0.0, 0.0), (6.0, 6.0, 6.0), "capacity"),       # 602^3 > 2^27 cells
        (2, 1e-3, (0.0, 0.0), (11.0, 11.0), "ok"),                     # 11 002^2 < 2^27: the last refusals are the limits'
    ]
    lines = [_geometry_line(dim, c, np.array(lo, F32), np.array(hi, F32)) for dim, c, lo, hi, _ in cases]
    for (dim, c, lo, hi, want), line in zip(cases, _run(driver, lines)):
        assert line.split()[0] == want, (dim, c, lo, hi, line)


# ------------------------------------------------------------------------------------------------ the cell of a point
def _axis_values(t, a):
    ext = t.ext[a]
    seams = [S.seam(t.origin[a], t.grid.inv_c, k) for k in (0, 1, ext - 1, ext)]
    return [v for s in seams for v in (s, S.below(s))] + [F32(np.nan), F32(np.inf), F32(-np.inf)]


def _expected_axis(rule, t, a, x):
    """(index, inside) of one coordinate under a key rule, the empty ring of 2D applied to the rule's index."""
    i, inside = S.index_mutant(rule, np.array([x], F32), t.origin[a], t.grid.inv_c, t.c, t.ext[a])
    i, inside = int(i[0]), bool(inside[0])
    return i, inside and RING[t.dim] <= i < t.ext[a] - RING[t.dim]


def test_cell_of_a_point_on_the_seams(driver):
    lines, cases = [], []
    for t in _seam_targets():
        mid = [F32(0.5 * (float(t.seams[a][2]) + float(t.seams[a][3]))) for a in range(t.dim)]     # inside, off the ring
        for a in range(t.dim):
            for x in _axis_values(t, a):
                p = list(mid)
                p[a] = x
                lines.append(_point_line(t.dim, t.c, t.origin, t.ext, p))
                cases.append((t, a, p))
    out = _run(driver, lines)
    differs = dict.fromkeys(MUTANTS, 0)
    for (t, a, p), line in zip(cases, out):
        got = line.split()
        want = [_expected_axis("rule", t, b, p[b]) for b in range(t.dim)]
        assert all(w[1] for b, w in enumerate(want) if b != a), t.name
        assert (got[0] == "in") == want[a][1], (t.name, a, p, line)
        if want[a][1]:
            assert [int(v) for v in got[1:1 + t.dim]] == [w[0] for w in want], (t.name, a, p, line)
        for m in MUTANTS:
            mi, min_ = _expected_axis(m, t, a, p[a])
            if min_ != want[a][1] or (min_ and mi != want[a][0]):
                differs[m] += 1
    assert all(differs[m] > 0 for m in MUTANTS), differs          # each mutant would have been caught


# ------------------------------------------------------------------------------------------------ the terms of a point
def _term_cloud(dim, c, centre):
    rng = np.random.default_rng([dim, int(c * 1000), int(abs(centre)), int(centre < 0)])
    return (centre + 3.0 * rng.normal(size=(N_TERM_POINTS, dim))).astype(F32)


@pytest.mark.parametrize("dim,c,centre", TERM_CLOUDS)
def test_terms_of_a_point(driver, dim, c, centre):
    P = _term_cloud(dim, c, centre)
    origin, ext = R.grid_geometry(P, c)
    out = _run(driver, [_point_line(dim, c, origin, ext, p) for p in P])
    assert all(line.startswith("in ") for line in out)            # no point is left out
    got = np.array([[int(v) for v in line.split()[1:]] for line in out], dtype=object)
    idx = ((P - origin[None, :]) * F32(1.0 / c)).astype(np.int64)                      # float32 arithmetic, then (int)f
    assert np.array_equal(got[:, :dim].astype(np.int64), idx)
    centres = R.cell_centres(origin, idx, c)         # (i + 0.5) c + o exactly, rounded once (cell_record_ref.centres)
    U = np.rint((P.astype(np.float64) - centres) * (2.0 ** 22 / c)).astype(np.int64)
    assert int(np.abs(U).max()) <= 1 << 21
    assert np.array_equal(got[:, dim:2 * dim].astype(np.int64), U)
    pairs = [(a, b) for a in range(dim) for b in range(a, dim)]
    terms = [[int(u) for u in row] + [int(row[a]) * int(row[b]) for a, b in pairs] for row in U]
    assert got[:, 2 * dim:].tolist() == terms
