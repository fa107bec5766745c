"""The exhaustive pose search's lattice and hit rules on the CPU: ndt2d_search_lattice_size against the numpy
restatement (gtsam_ndt_amd/search.py), select_hits on hand-made volumes, and the new structs' layout."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import search

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEG = math.pi / 180.0


def _lib_dims(lib, window):
    w = L.SearchWindow2D()
    for a in range(3):
        w.center[a], w.half_extent[a], w.step[a] = window[0][a], window[1][a], window[2][a]
    dims = (C.c_int32 * 3)()
    st = lib.ndt2d_search_lattice_size(C.byref(w), C.cast(dims, C.c_void_p))
    return st, tuple(dims)


@pytest.mark.parametrize("window", [
    ((0.0, 0.0, 0.0), (3.0, 3.0, math.pi), (0.1, 0.1, DEG)),            # scenario A: 61 x 61 x 360
    ((1.0, -2.0, 0.3), (0.3, 0.3, 0.1), (0.1, 0.1, 0.05)),              # 0.3 / 0.1 = 2.9999999999999996: the 1e-9 edge
    ((0.0, 0.0, 0.0), (0.0, 0.7, 0.0), (0.2, 0.1, 0.1)),                # pinned axes
    ((0.0, 0.0, 3.0), (0.5, 0.5, 4.0), (0.5, 0.5, 2.0 * DEG)),          # full turn, 180 headings
    ((0.0, 0.0, 0.0), (0.5, 0.5, math.pi), (0.5, 0.5, 7.0)),            # a step wider than the turn: one heading
    ((0.0, 0.0, 0.0), (0.5, 0.5, math.pi - 1e-12), (0.5, 0.5, 0.5)),    # just short of a full turn: not cyclic
])
def test_lattice_size_matches_the_restatement(ndt_lib, window):
    st, d = _lib_dims(ndt_lib, window)
    assert st == L.NDT_OK
    want, cyclic = search.dims(window)
    assert d == want
    xs, ys, th = search.lattice(window)
    assert (th.size, ys.size, xs.size) == d
    assert np.all(th > -math.pi) and np.all(th <= math.pi)
    if cyclic:
        assert window[1][2] >= math.pi


def test_lattice_values():
    xs, ys, th = search.lattice(((1.0, -2.0, 0.3), (0.3, 0.3, 0.1), (0.1, 0.1, 0.05)))
    assert xs.size == 7 and xs[3] == 1.0 and xs[0] == 1.0 + (-3.0) * 0.1
    assert th.size == 5 and th[2] == 0.3
    _, _, th = search.lattice(((0.0, 0.0, 3.0), (0.0, 0.0, math.pi), (1.0, 1.0, 90.0 * DEG)))
    assert th.size == 4 and th[0] == 3.0 and th[1] == float(search.wrap(3.0 + 0.5 * math.pi))


def test_capacity_and_invalid_windows(ndt_lib):
    big = ((0.0, 0.0, 0.0), (50.0, 50.0, math.pi), (0.01, 0.01, 0.1))
    assert _lib_dims(ndt_lib, big)[0] == L.NDT_ERR_CAPACITY
    with pytest.raises(search.CapacityError):
        search.dims(big)
    edge = ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (2.0 ** -25, 1.0, 1.0))     # 2^26 + 1 poses on one axis
    assert _lib_dims(ndt_lib, edge)[0] == L.NDT_ERR_CAPACITY
    for bad in [((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.1, 0.1)),
                ((0.0, 0.0, 0.0), (-1.0, 1.0, 1.0), (0.1, 0.1, 0.1)),
                ((math.nan, 0.0, 0.0), (1.0, 1.0, 1.0), (0.1, 0.1, 0.1)),
                ((0.0, 0.0, 0.0), (1.0, math.inf, 1.0), (0.1, 0.1, 0.1))]:
        assert _lib_dims(ndt_lib, bad)[0] == L.NDT_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            search.dims(bad)


W1 = ((0.0, 0.0, 0.0), (2.0, 1.0, 0.1), (1.0, 1.0, 0.1))                  # 3 x 3 x 5, not cyclic


def test_select_hits_ties_go_to_the_lower_index():
    v = np.zeros((3, 3, 5), dtype=np.float32)
    v[1, 1, 1] = 2.0
    v[1, 1, 2] = 2.0                                                    # a tie with a neighbour: index 21 beats 22
    v[0, 0, 4] = 1.0
    hits = search.select_hits(v, W1, k=8, min_sep=(0.0, 0.0))
    assert [h.index for h in hits] == [21, 4]
    assert hits[0].pose == (-1.0, 0.0, 0.0) and hits[0].score == 2.0
    assert not search.peaks(np.zeros((3, 3, 3), np.float32), False).any()   # zeros are never peaks


def test_select_hits_wraps_only_a_cyclic_axis():
    v = np.zeros((4, 1, 1), dtype=np.float32)
    v[:, 0, 0] = [3.0, 1.0, 2.0, 4.0]
    lin = ((0.0, 0.0, 0.0), (0.0, 0.0, 1.5), (1.0, 1.0, 1.0))          # 4 headings? no: 2 floor(1.5) + 1 = 3
    assert search.dims(lin)[0] == (3, 1, 1)
    cyc = ((0.0, 0.0, 0.0), (0.0, 0.0, math.pi), (1.0, 1.0, 0.5 * math.pi))
    assert search.dims(cyc) == ((4, 1, 1), True)
    # cyclic: heading 0 (3.0) is a neighbour of heading 3 (4.0) and loses to it
    assert [h.index for h in search.select_hits(v, cyc, 8, (0.0, 0.0))] == [3]
    v3 = np.array([3.0, 1.0, 4.0], dtype=np.float32).reshape(3, 1, 1)
    assert [h.index for h in search.select_hits(v3, lin, 8, (0.0, 0.0))] == [2, 0]


def test_select_hits_separation_needs_both_distances():
    win = ((0.0, 0.0, 0.0), (4.0, 0.0, 0.0), (1.0, 1.0, 1.0))           # nine x positions, one heading
    v = np.zeros((1, 1, 9), dtype=np.float32)
    v[0, 0, [0, 2, 4, 6, 8]] = [5.0, 4.0, 3.0, 2.0, 1.0]
    assert [h.index for h in search.select_hits(v, win, 8, (0.0, 0.0))] == [0, 2, 4, 6, 8]
    assert [h.index for h in search.select_hits(v, win, 8, (2.5, 0.1))] == [0, 4, 8]
    assert [h.index for h in search.select_hits(v, win, 2, (2.5, 0.1))] == [0, 4]
    # the rotation gap is 0 < min_sep_rot only when it is > 0: a zero rotation threshold suppresses nothing
    assert [h.index for h in search.select_hits(v, win, 8, (2.5, 0.0))] == [0, 2, 4, 6, 8]
    # heading separation is wrapped: -pi + 0.1 and pi are 0.1 apart
    cyc = ((0.0, 0.0, 0.0), (1.0, 0.0, math.pi), (2.0, 1.0, 2.0 * math.pi / 3.0))
    (nt, ny, nx), _ = search.dims(cyc)
    assert (nt, ny, nx) == (3, 1, 1)


def test_search_structs_match_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ndt_hip.h"\n'
                    'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(ndt2d_search_window),'
                    'offsetof(ndt2d_search_window, half_extent), offsetof(ndt2d_search_window, step),'
                    'offsetof(ndt2d_search_window, min_sep_trans), offsetof(ndt2d_search_window, min_sep_rot),'
                    'sizeof(ndt2d_search_hit), offsetof(ndt2d_search_hit, score), offsetof(ndt2d_search_hit, index));'
                    'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["g++", "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    W, H = L.SearchWindow2D, L.SearchHit2D
    assert out == [C.sizeof(W), W.half_extent.offset, W.step.offset, W.min_sep_trans.offset, W.min_sep_rot.offset,
                   C.sizeof(H), H.score.offset, H.index.offset]
    assert C.sizeof(W) == 88 and C.sizeof(H) == 32
