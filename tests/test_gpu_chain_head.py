"""k_iterate's results, bit for bit, against a recording of the build before the head of the launch was reordered
(partial-row loads ahead of the scalar batch, tests/golden/chain_head.npz from tests/golden/make_chain_head_golden.py).
A change to the order of loads and waits must not move a single bit of pose, H, g, score, iterations, n_hit or status;
a load that lands on the wrong row, a row consumed before it arrived or a wave folding rows it does not own would.

Cases and shapes: tests/chain_head_cases.py (scans of 4 097, 65 537 and 300 000 points against a 100 000-point target;
1, 2 and 30 fixed iterations and converged mode; Newton Hessian; four overlapping grids; two alignments per handle and
two asynchronous ones on the two launch chains)."""
import os

import numpy as np
import pytest

import chain_head_cases as cc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chain_head.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def world():
    return cc.make_world()


@pytest.fixture(scope="module")
def dev_scan(gpu_lib, world):
    import torch
    dev = (torch.from_numpy(world["sx"]).cuda(), torch.from_numpy(world["sy"]).cuda())
    torch.cuda.synchronize()
    return dev


def test_fixture_covers_the_cases(golden):
    assert sorted(golden) == sorted(f"{c[0]}/{f}" for c in cc.CASES for f in cc.FIELDS)


@pytest.mark.parametrize("case", cc.CASES, ids=[c[0] for c in cc.CASES])
def test_results_are_bit_identical_to_the_recording(gpu_lib, world, dev_scan, golden, case):
    name, _, k, _, _ = case
    got = cc.run_case(world, dev_scan, case)
    assert got["iterations"].shape == (3 if k > 0 else 2,)
    if k > 0:
        assert got["iterations"].tolist() == [k] * 3
    for f in cc.FIELDS:
        want = golden[f"{name}/{f}"]
        print(name, f, "got", got[f].tolist(), "want", want.tolist())
        assert got[f].dtype == want.dtype and got[f].shape == want.shape
        assert got[f].tobytes() == want.tobytes(), f"{name}: {f} differs from the recording"
