"""The single-scan chain hands a launch's sums to the next as three 16-byte entries per workgroup (the packed
AlignDyn::partials) and folds them with three waves of four sums: every result must be, bit for bit, what the
row-per-sum table returned.  The reference is tests/golden/packed_partials.npz, recorded from the library before the
change (tests/golden/make_packed_partials_golden.py).  Cases and shapes: tests/packed_partials_cases.py (a 20 000-point
target, scans of 4 097 to 6 000 points, K <= 6)."""
import os

import numpy as np
import pytest

import packed_partials_cases as pc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "packed_partials.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def world():
    return pc.make_world()


@pytest.fixture(scope="module")
def dev(gpu_lib, world):
    return pc.to_device(world)


@pytest.fixture(scope="module")
def results(gpu_lib, world, dev):
    """Every case once, shared by the tests below."""
    return {case[0]: pc.run_case(world, dev, case) for case in pc.CASES}


def test_fixture_covers_the_cases(golden):
    assert sorted(golden) == sorted(f"{c[0]}/{f}" for c in pc.CASES for f in pc.FIELDS)


@pytest.mark.parametrize("case", pc.CASES, ids=pc.CASE_IDS)
def test_results_are_bit_identical_to_the_recording(results, golden, case):
    got = results[case[0]]
    for f in pc.FIELDS:
        want = golden[f"{case[0]}/{f}"]
        print(case[0], f, "got", got[f].tolist(), "want", want.tolist())
        assert got[f].dtype == want.dtype and got[f].shape == want.shape, (case[0], f)
        assert got[f].tobytes() == want.tobytes(), f"{case[0]}: {f} differs"


def test_the_cases_do_what_they_are_for(results):
    """The recorded alignments reach the situations they were chosen for."""
    r = results
    # a 4 097-point scan: 17 (256 threads) or 5 (1024 threads) workgroups have points, the rest hand over zeros; all
    # its points are counted
    for name in ("gn_k3", "newton_k3", "gn_overlap4_k3", "wide_gn_k3", "wide_newton_overlap4_k3", "k_begin_k3", "k1"):
        assert r[name]["status"][0] == 0 and 2000 < r[name]["n_hit"][0] <= 4 * 4097, (name, r[name]["n_hit"][0])
    # two chains give what one chain gives
    for f in pc.FIELDS:
        assert r["async_one_lane"][f].tobytes() == r["async_two_lanes"][f].tobytes(), f
    # k_begin + k_iterate gives what k_iterate_first gives; so do plain launches
    for f in pc.FIELDS:
        assert r["k_begin_k3"][f][:2].tobytes() == r["gn_k3"][f][:2].tobytes(), f
        assert r["no_graph_k3"][f][:1].tobytes() == r["gn_k3"][f][:1].tobytes(), f
    # converged mode: the chunk length does not show; few and many iterations
    for f in pc.FIELDS:
        assert r["converged_chunk2"][f].tobytes() == r["converged_chunk8"][f].tobytes(), f
    it = r["converged_chunk8"]["iterations"].tolist()
    assert it[0] < it[1] and it[1] > 8, it
    # an alignment that ended at its first solve, then a normal one
    for name in ("too_few_hits", "too_few_hits_converged"):
        assert r[name]["status"][0] == pc.fc.NDT_TOO_FEW_HITS and r[name]["iterations"][0] == 0, name
        assert r[name]["status"][1] == 0 and r[name]["n_hit"][1] > 2000, name
    # the trace has a row per update, and its last row is the alignment
    t = r["trace_k6"]
    assert t["iterations"].tolist() == [6] + list(range(1, 7)) + list(range(1, 7)) + [6]
    for f in ("pose", "H", "g", "score", "n_hit"):
        assert t[f][3:4].tobytes() == r["gn_k3"][f][0:1].tobytes(), f        # 3 updates of the s4097 / I0 trace = K = 3
    assert len(r["trace_converged"]["iterations"]) > 8
    # an evaluation off the grid finds nothing
    assert r["eval"]["n_hit"][4] == 0 and r["eval"]["n_hit"][0] > 2000
