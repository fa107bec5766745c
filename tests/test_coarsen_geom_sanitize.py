"""The host arithmetic of submap coarsening (the lattice of docs/ALGORITHM.md section 2.17: k0, K0, the coarse extent and
origin; gtsam_ndt_amd/csrc/ndt_coarsen_geom.hpp) in a stand-alone program under gcc's AddressSanitizer and
UndefinedBehaviorSanitizer, against tests/map_coarsen_ref.py: negative origins, the smallest grids, extents at the
2^27-cell limit, and origins no grid of the library has (refused, not undefined)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import map_coarsen_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("san") / "coarsen_geom")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gtsam_ndt_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "coarsen_geom_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


def _run(driver, cases):
    text = "".join(f"{float(o)!r} {float(c)!r} {w} {f}\n" for o, c, w, f in cases)
    p = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    return p.stdout.splitlines()


def test_lattice_arithmetic_is_clean_and_agrees_with_the_reference(driver):
    cases = []
    for f in (2, 4):
        for c in (0.5, 1.0, 0.3):
            for k0 in (-1000003, -9, -8, -7, -6, -5, -4, -3, -2, -1, 0, 1, 2, 3, 4, 5, 6, 7, 1000001):
                for w in (1, 2, 3, 4, 5, 13, 300, (1 << 27) // 3, 1 << 27):
                    cases.append((np.float32(k0 * c), c, w, f))
    out = _run(driver, cases)
    assert len(out) == len(cases) + 1
    for (o, c, w, f), line in zip(cases, out):
        k0, K0, off, extent = R.coarsen_axis(o, c, w, f)
        bits = int(np.float32(K0 * c).view(np.uint32))
        assert line == f"ok {k0} {K0} {off} {extent} {bits}", (o, c, w, f, line)
        assert K0 % f == 0 and f - 1 <= off <= 2 * f - 2 and 2 <= extent <= w // f + 3
    assert out[-1] == "factors 2 4 0 0 2"


def test_what_is_no_lattice_is_refused(driver):
    big = float(np.finfo(np.float32).max)
    cases = [(big, 0.5, 10, 2), (-big, 1e-3, 10, 4), (float("nan"), 0.5, 10, 2), (float("inf"), 0.5, 10, 2),
             (1.0, 0.5, 10, 3), (1.0, 0.5, 10, 8), (1.0, 0.5, 0, 2), (1.0, 0.0, 10, 2), (1.0, -1.0, 10, 2), (3e12, 1.0, 10, 2)]
    assert _run(driver, cases)[:-1] == ["refused"] * len(cases)
