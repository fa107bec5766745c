"""The exhaustive 3D pose search's lattice and hit rules on the CPU: ndt3d_search_lattice_size against the numpy
restatement (gtsam_ndt_amd/search.py) for 3D windows, select_hits with a 6-vector centre on a hand-made volume, and
the new structs' layout."""
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
    w = L.SearchWindow3D()
    for a in range(6):
        w.center[a] = window[0][a]
    for a in range(3):
        w.half_extent[a], w.step[a] = window[1][a], window[2][a]
    dims = (C.c_int32 * 3)()
    st = lib.ndt3d_search_lattice_size(C.byref(w), C.cast(dims, C.c_void_p))
    return st, tuple(dims)


@pytest.mark.parametrize("window", [
    ((4.5, -3.7, 0.0, 0.0, 0.0, 2.0), (3.0, 3.0, math.pi), (0.25, 0.25, DEG)),           # the relocalisation: 25 x 25 x 360
    ((1.0, -2.0, 0.5, 0.01, -0.02, 0.3), (0.3, 0.3, 0.1), (0.1, 0.1, 0.05)),             # the 1e-9 edge of 0.3 / 0.1
    ((0.0, 0.0, 1.0, 0.0, 0.0, 0.0), (0.0, 0.7, 0.0), (0.2, 0.1, 0.1)),                  # pinned axes
    ((0.0, 0.0, 0.0, 0.1, 0.1, 3.0), (0.5, 0.5, 4.0), (0.5, 0.5, 2.0 * DEG)),            # full turn, 180 yaws
    ((0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.5, 0.5, math.pi), (0.5, 0.5, 7.0)),              # a step wider than the turn
    ((0.0, 0.0, 0.0, 0.0, 0.0, 0.0), (0.5, 0.5, math.pi - 1e-12), (0.5, 0.5, 0.5)),      # just short of a full turn
    ((0.0, 0.0, 7.0, 3.0, 3.0, 0.0), (1.0, 1.0, 0.2), (0.5, 0.5, 0.1)),                  # the pinned values do not count
])
def test_lattice_size_matches_the_restatement(ndt_lib, window):
    st, d = _lib_dims(ndt_lib, window)
    assert st == L.NDT_OK
    want, cyclic = search.dims(window)
    assert d == want
    # the lattice of a 3D window is that of the 2D window over its searched axes
    c = window[0]
    flat = ((c[0], c[1], c[5]), window[1], window[2])
    assert search.dims(flat) == (want, cyclic)
    for a, b in zip(search.lattice(window), search.lattice(flat)):
        assert np.array_equal(a, b)
    xs, ys, th = search.lattice(window)
    assert (th.size, ys.size, xs.size) == d
    assert np.all(th > -math.pi) and np.all(th <= math.pi)


def test_capacity_and_invalid_windows(ndt_lib):
    z = (0.0,) * 6
    big = (z, (50.0, 50.0, math.pi), (0.01, 0.01, 0.1))
    assert _lib_dims(ndt_lib, big)[0] == L.NDT_ERR_CAPACITY
    with pytest.raises(search.CapacityError):
        search.dims(big)
    for bad in [(z, (1.0, 1.0, 1.0), (0.0, 0.1, 0.1)),
                (z, (-1.0, 1.0, 1.0), (0.1, 0.1, 0.1)),
                (z, (1.0, math.inf, 1.0), (0.1, 0.1, 0.1)),
                ((math.nan, 0.0, 0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.1, 0.1, 0.1)),
                ((0.0, 0.0, math.nan, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.1, 0.1, 0.1)),       # z
                ((0.0, 0.0, 0.0, math.inf, 0.0, 0.0), (1.0, 1.0, 1.0), (0.1, 0.1, 0.1)),       # roll
                ((0.0, 0.0, 0.0, 0.0, math.nan, 0.0), (1.0, 1.0, 1.0), (0.1, 0.1, 0.1)),       # pitch
                ((0.0, 0.0, 0.0, 0.0, 0.0, math.nan), (1.0, 1.0, 1.0), (0.1, 0.1, 0.1))]:      # yaw
        assert _lib_dims(ndt_lib, bad)[0] == L.NDT_ERR_INVALID_ARG
        with pytest.raises(ValueError):
            search.dims(bad)
    dims = (C.c_int32 * 3)()
    assert ndt_lib.ndt3d_search_lattice_size(None, C.cast(dims, C.c_void_p)) == L.NDT_ERR_INVALID_ARG
    w = L.SearchWindow3D()
    assert ndt_lib.ndt3d_search_lattice_size(C.byref(w), None) == L.NDT_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        search.dims(((0.0, 0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.1, 0.1, 0.1)))                 # neither 3 nor 6 values


def test_select_hits_carries_the_pinned_coordinates():
    c = (1.0, -2.0, 0.25, 0.01, -0.02, 0.5)
    win = (c, (2.0, 1.0, 0.1), (1.0, 1.0, 0.1))                          # 3 yaws x 3 x 5, not cyclic
    assert search.dims(win) == ((3, 3, 5), False)
    v = np.zeros((3, 3, 5), dtype=np.float32)
    v[1, 1, 1] = 2.0
    v[1, 1, 2] = 2.0                                                    # a tie with a neighbour: index 21 beats 22
    v[0, 0, 4] = 1.0
    v[2, 2, 4] = 0.5
    hits = search.select_hits(v, win, k=8, min_sep=(0.0, 0.0))
    assert [h.index for h in hits] == [21, 4, 44]
    assert hits[0].pose == (0.0, -2.0, 0.25, 0.01, -0.02, 0.5) and hits[0].score == 2.0
    assert hits[1].pose == (3.0, -3.0, 0.25, 0.01, -0.02, 0.4)
    assert hits[2].pose == (3.0, -1.0, 0.25, 0.01, -0.02, 0.6)
    # the same volume under the 2D window over the searched axes: the same hits, 3-vector poses
    flat = search.select_hits(v, ((c[0], c[1], c[5]), win[1], win[2]), k=8, min_sep=(0.0, 0.0))
    assert [(h.pose[0], h.pose[1], h.pose[5], h.score, h.index) for h in hits] == [(*h.pose, h.score, h.index) for h in flat]
    # separation uses dx, dy and the wrapped yaw (the last component), never the pinned coordinates
    assert [h.index for h in search.select_hits(v, win, 8, (10.0, 0.15))] == [21]
    assert [h.index for h in search.select_hits(v, win, 8, (10.0, 0.05))] == [21, 4, 44]
    assert [h.index for h in search.select_hits(v, win, 8, (2.5, 0.15))] == [21, 4, 44]
    cyc = ((0.0, 0.0, 9.0, 9.0, 9.0, 3.0), (0.0, 0.0, math.pi), (1.0, 1.0, 0.5 * math.pi))
    v4 = np.array([3.0, 1.0, 2.0, 4.0], dtype=np.float32).reshape(4, 1, 1)
    got = search.select_hits(v4, cyc, 8, (0.0, 0.0))
    assert [h.index for h in got] == [3]                                # yaw 0 is a neighbour of yaw 3 on a cyclic axis
    assert got[0].pose == (0.0, 0.0, 9.0, 9.0, 9.0, float(search.wrap(3.0 + 1.5 * math.pi)))


def test_search3d_structs_match_the_header(tmp_path):
    prog = tmp_path / "sz.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ndt_hip.h"\n'
                    'int main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\\n", sizeof(ndt3d_search_window),'
                    'offsetof(ndt3d_search_window, half_extent), offsetof(ndt3d_search_window, step),'
                    'offsetof(ndt3d_search_window, min_sep_trans), offsetof(ndt3d_search_window, min_sep_rot),'
                    'sizeof(ndt3d_search_hit), offsetof(ndt3d_search_hit, score), offsetof(ndt3d_search_hit, index),'
                    'NDT_ABI_VERSION);'
                    'return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["g++", "-x", "c++", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)],
                   check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    W, H = L.SearchWindow3D, L.SearchHit3D
    assert out == [C.sizeof(W), W.half_extent.offset, W.step.offset, W.min_sep_trans.offset, W.min_sep_rot.offset,
                   C.sizeof(H), H.score.offset, H.index.offset, 1]
    assert C.sizeof(W) == 112 and C.sizeof(H) == 56


def test_cpp_adapter_exposes_the_3d_search(tmp_path):
    src = tmp_path / "s.cpp"
    src.write_text('#include "ndt_matcher_hip.hpp"\n'
                   'int main(){ auto a = &ndt::NdtMatcherHip3::searchDev; auto b = &ndt::NdtMatcherHip3::searchAlignDev;\n'
                   '  ndt::NdtMatcherHip3::SearchMatch m; (void)a; (void)b; (void)m; return 0; }\n')
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                    "-o", str(tmp_path / "s.o")], check=True)
