"""The map-to-map pose search in the float64 restatement alone (tests/d2d_search_ref.py, tests/d2d_ref.py and
gtsam_ndt_amd/search.py; docs/ALGORITHM.md section 2.15): the vectorised volume is the restatement's score pose by pose,
and the search does what it is for - a submap pair whose guess lies outside the local optimiser's basin is brought
together by the best lattice pose, refined.  Also: the three entry points exist in the header, the library and the
bindings."""
import math
import os
import re

import numpy as np
import pytest

import d2d_ref as R
import d2d_search_ref as S
from gtsam_ndt_amd import search, synth
from oracle import ndt2d as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEG = math.pi / 180.0
NAMES = ("ndt2d_search_map", "ndt2d_search_map_scores", "ndt2d_search_align_map")
OFFSET = (1.1, -0.9, 0.35)               # the guess: the generating pose plus this


def _dist(p, q):
    return math.hypot(p[0] - q[0], p[1] - q[1]), abs(float(search.wrap(p[2] - q[2])))


@pytest.fixture(scope="module")
def room50():
    d = synth.make_pair(2, n_tgt=20_000, n_src=20_000)
    prm = O.NdtParams()
    tgt, _ = R.build_map(d["tx"], d["ty"], prm)
    _, comps = R.build_map(d["sx"], d["sy"], prm)
    return d, tgt, comps, prm


def test_the_vectorised_volume_is_the_restatement_pose_by_pose(room50):
    d, tgt, comps, prm = room50
    window = search.Window(d["init"], (0.5, 0.25, 0.2), (0.25, 0.25, 0.1))
    assert search.dims(window)[0] == (5, 3, 5)
    fast, slow = S.volume(tgt, comps, window, prm), S.volume_by_loop(tgt, comps, window, prm)
    assert fast.shape == slow.shape == (5, 3, 5)
    assert slow.max() > 10.0
    # the same terms, summed by numpy over another shape: rounding of a float64 sum of ~1000 positive terms
    assert np.max(np.abs(fast - slow)) <= 1e-12 * slow.max()
    # and off the map: exact zeros on both sides
    far = search.Window((500.0, 500.0, 0.0), (0.25, 0.25, 0.1), (0.25, 0.25, 0.1))
    assert not S.volume(tgt, comps, far, prm).any() and not S.volume_by_loop(tgt, comps, far, prm).any()


def test_the_search_closes_a_loop_the_local_optimiser_cannot(room50):
    d, tgt, comps, prm = room50
    true = d["pose"]
    guess = tuple(a + b for a, b in zip(true, OFFSET))
    local = R.align(tgt, comps, guess, prm)
    dt, dr = _dist(local["pose"], true)
    print(f"{comps.n} components, {tgt.n_valid} target cells; local run from the guess: status {local['status']}, "
          f"{dt:.3f} m / {dr:.3f} rad from the generating pose")
    assert dt > 1.0
    window = search.Window(guess, (2.0, 2.0, math.pi), (0.25, 0.25, 4.0 * DEG))
    assert search.dims(window)[0] == (90, 17, 17)
    vol = S.volume(tgt, comps, window, prm)
    hits = search.select_hits(vol.astype(np.float32), window, k=4)
    assert len(hits) == 4
    print("hits:", [(tuple(round(v, 4) for v in h.pose), round(h.score, 1)) for h in hits])
    best = R.align(tgt, comps, hits[0].pose, prm)
    dt, dr = _dist(best["pose"], true)
    print(f"best hit refined: status {best['status']}, {best['iterations']} iterations, {dt:.4f} m / {dr:.2e} rad off")
    assert best["status"] == O.NDT_OK
    assert dt < 0.05 and dr < 0.005
    # what holds the device to a pose: the restatement's own float32 and float64 runs from every hit used
    worst = 0.0
    for h in hits:
        a, b = R.align(tgt, comps, h.pose, prm, mirror32=True), R.align(tgt, comps, h.pose, prm)
        assert a["status"] == b["status"]
        worst = max(worst, float(np.max(np.abs(np.array(a["pose"]) - np.array(b["pose"])))))
    print(f"float32 vs float64 refinements of the {len(hits)} hits: at most {worst:.2e} apart")
    assert worst < 2.5e-5


def test_a_map_searched_against_itself_peaks_at_the_centre():
    """The premise of the GPU self-search test: the restatement's maximum over a window centred on the identity is
    the centre pose, and it is unique."""
    d = synth.make_pair(1)
    prm = O.NdtParams()
    tgt, comps = R.build_map(d["tx"], d["ty"], prm)
    window = search.Window((0.0, 0.0, 0.0), (0.5, 0.5, math.pi), (0.1, 0.1, 10.0 * DEG))
    (nt, ny, nx), _ = search.dims(window)
    vol = S.volume(tgt, comps, window, prm)
    top = np.sort(vol.reshape(-1))[::-1]
    centre = (0 * ny + (ny - 1) // 2) * nx + (nx - 1) // 2
    print(f"self-search: maximum {top[0]:.3f} at index {int(np.argmax(vol))} (centre {centre}), next {top[1]:.3f}")
    assert int(np.argmax(vol)) == centre
    assert top[0] == pytest.approx(prm.d1 * comps.n, rel=1e-12) and top[1] < 0.9 * top[0]


def test_the_three_entry_points_are_declared_exported_and_bound(ndt_lib):
    from gtsam_ndt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ndt_hip.h")).read(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\bint32_t\s+%s\s*\(" % n, src), f"{n} is not declared in ndt_hip.h"
        assert hasattr(ndt_lib, n), f"{n} is not exported"
        assert n in _lib.SIGNATURES, f"{n} is not bound"
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    for m in ("search_map", "search_map_scores", "search_align_map"):
        assert callable(getattr(NdtMatcher2D, m))
    import adapter_calls as AC                                  # the C++ adapter's call record
    assert "ndt2d_search_align_map" in AC.calls()["NdtMatcherHip.searchAlignMap"]
