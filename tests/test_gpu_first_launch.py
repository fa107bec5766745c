"""The first launch of a 2D single-scan chain carries the call's arguments itself (k_iterate_first; no k_begin): the
results must be, bit for bit, what the chain behind k_begin returned.  Three references:
  * tests/golden/first_launch.npz, recorded from the library before the change (tests/golden/make_first_launch_golden.py);
  * the same build with NDT_TUNE_FUSED_BEGIN = 0, which runs k_begin and K + 1 launches;
  * for fixed-iteration cases, the last row of ndt2d_align_trace, which always runs that old protocol.
Cases and shapes: tests/first_launch_cases.py (a 20 000-point target, scans of 4 097 to 6 000 points, K <= 6)."""
import os

import numpy as np
import pytest

import first_launch_cases as fc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "first_launch.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def world():
    return fc.make_world()


@pytest.fixture(scope="module")
def dev(gpu_lib, world):
    return fc.to_device(world)


@pytest.fixture(scope="module")
def fused_results(gpu_lib, world, dev):
    """Every case once with the fused first launch (the default, set explicitly), shared by the tests below."""
    return {case[0]: fc.run_case(world, dev, case, fused=1) for case in fc.CASES}


def same_bits(a, b, what):
    for f in fc.FIELDS:
        print(what, f, "got", a[f].tolist(), "want", b[f].tolist())
        assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape, (what, f)
        assert a[f].tobytes() == b[f].tobytes(), f"{what}: {f} differs"


def test_fixture_covers_the_cases(golden):
    assert sorted(golden) == sorted(f"{c[0]}/{f}" for c in fc.CASES for f in fc.FIELDS)


def test_fused_begin_is_the_default_and_checks_its_value(gpu_lib, world, dev):
    from gtsam_ndt_amd._lib import NdtError
    case = fc.CASES[fc.CASE_IDS.index("stale_sync")]
    same_bits(fc.run_case(world, dev, case, fused=None), fc.run_case(world, dev, case, fused=1), "default")
    with fc.open_matcher(world, case, None) as m:
        for bad in (-1, 2):
            with pytest.raises(NdtError):
                m.set_tuning("fused_begin", bad)


@pytest.mark.parametrize("case", fc.CASES, ids=fc.CASE_IDS)
def test_results_are_bit_identical_to_the_recording(fused_results, golden, case):
    got = fused_results[case[0]]
    assert got["iterations"].shape == (fc.n_results(case),)
    same_bits(got, {f: golden[f"{case[0]}/{f}"] for f in fc.FIELDS}, case[0])


@pytest.mark.parametrize("case", fc.CASES, ids=fc.CASE_IDS)
def test_fused_equals_k_begin_protocol(world, dev, fused_results, case):
    same_bits(fused_results[case[0]], fc.run_case(world, dev, case, fused=0), case[0])


TRACED = [c for c in fc.CASES if fc.is_fixed(c) and any(step[0] == "sync" for step in c[3])]


@pytest.mark.parametrize("case", TRACED, ids=[c[0] for c in TRACED])
def test_fixed_cases_equal_the_last_trace_row(world, fused_results, case):
    got = fused_results[case[0]]
    rows = fc.run_trace(world, case, fused=1)
    assert rows
    for j, r in rows.items():
        same_bits({f: got[f][j:j + 1] for f in fc.FIELDS}, fc.pack([r]), f"{case[0]} step {j}")


def test_the_cases_do_what_they_are_for(fused_results):
    """The recorded alignments reach the situations they were chosen for."""
    r = fused_results
    K = {c[0]: c[1].get("fixed_iterations", 0) for c in fc.CASES}
    for name in ("stale_sync", "stale_async", "k1", "no_graph_k3", "wide_k3"):
        assert r[name]["status"].tolist() == [0] * len(r[name]["status"]), name
        assert r[name]["iterations"].tolist() == [K[name]] * len(r[name]["iterations"]), name
    # an alignment that ended at its first solve, then a normal one
    for name in ("too_few_hits_fixed", "too_few_hits_converged"):
        assert r[name]["status"][0] == fc.NDT_TOO_FEW_HITS and r[name]["iterations"][0] == 0, name
        assert r[name]["status"][1] == 0 and r[name]["n_hit"][1] > 4000, name
    assert r["too_few_hits_fixed"]["status"][2] == 0
    # converged mode: few and many iterations around the chunk lengths
    for name in ("converged_chunk2", "converged_chunk8"):
        it = r[name]["iterations"].tolist()
        assert r[name]["status"].tolist() == [0, 0, 0, 0], name
        assert it[0] < it[1] and it[2] < it[3] and it[1] > 8, (name, it)
    assert r["converged_chunk2"]["iterations"].tolist() == r["converged_chunk8"]["iterations"].tolist()
    # the wrapped angle comes back wrapped
    assert np.all(np.abs(r["yaw_wrap"]["pose"][:, 2]) <= np.pi)
    assert np.abs(r["yaw_wrap"]["pose"][2] - r["yaw_wrap"]["pose"][3]).max() < 1e-6      # a whole turn either way
    # the second line-search alignment repeats the first: nothing of the first call's ls[] survives
    for name in ("line_search_k6", "line_search_converged"):
        for f in fc.FIELDS:
            assert r[name][f][0].tobytes() == r[name][f][1].tobytes(), (name, f)
