"""The first launch of a 3D chain carries the call's arguments itself (k_iterate3_first; no k_begin3): the results must
be, bit for bit, what the chain behind k_begin3 returned.  References as in test_gpu_first_launch.py:
tests/golden/first_launch3d.npz, recorded from the library before the change; the same build with
NDT_TUNE_FUSED_BEGIN = 0; for fixed-iteration cases the last row of ndt3d_align_trace, which always runs the old
protocol.  Cases and shapes: tests/first_launch3d_cases.py (4 096- and 3 000-point scans, K <= 4)."""
import os

import numpy as np
import pytest

import first_launch3d_cases as fc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "first_launch3d.npz")


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
    case = fc.CASES[fc.CASE_IDS.index("k3")]
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
def test_fused_equals_k_begin3_protocol(world, dev, fused_results, case):
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
    r = fused_results
    for name, k in (("k3", 3), ("k1", 1), ("k4_newton", 4)):
        assert r[name]["status"].tolist() == [0] * len(r[name]["status"]), name
        assert r[name]["iterations"].tolist() == [k] * len(r[name]["iterations"]), name
    for name in ("too_few_hits_k2", "too_few_hits_converged"):
        assert r[name]["status"][0] == fc.NDT_TOO_FEW_HITS and r[name]["iterations"][0] == 0, name
        assert r[name]["status"][1] == 0 and r[name]["n_hit"][1] > 1000, name
    assert r["converged"]["status"].tolist() == [0, 0, 0]
    assert np.all(np.abs(r["angles_wrap_k2"]["pose"][:, 3:]) <= np.pi)
    for f in fc.FIELDS:
        assert r["line_search_converged"][f][0].tobytes() == r["line_search_converged"][f][1].tobytes(), f
