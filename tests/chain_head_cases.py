"""The alignments of tests/test_gpu_chain_head.py and of tests/golden/make_chain_head_golden.py, which records what
they return (tests/golden/chain_head.npz).  One definition, so that the fixture and the test cannot drift apart.

The world: a 100 000-point target of the 50 m room (make_pair(2)) and prefixes of one 300 000-point scan of it (the
generator emits points in random order, so a prefix is a scan of its own).  Scan sizes are the edges of k_iterate's
launch shapes:
    4 097    the smallest scan that runs k_iterate and not k_align_small: most of the 256 workgroups have no point
             and contribute a zero partial row
    65 537   256 workgroups x 256 threads + 1: exactly one thread holds a second point
    300 000  the default wide_threshold: the first scan on 1024-thread workgroups
K > 0 is the fixed-iteration graph of K + 1 launches (K = 1 and 2: both parities of the last launch; every chain starts
with the launch without partials), K = 0 the converged mode (chunks of launches: the finishing launch and the ones
past the end).  Every case aligns twice on the same handle, from two initial poses: the second alignment starts on
state and partial tables the first one left dirty.  Fixed-iteration cases then run the same two as asynchronous calls,
which puts the second on the handle's other launch chain."""
import numpy as np

from gtsam_ndt_amd import synth

SIZES = (4097, 65537, 300000)
N_TARGET = 100_000
SECOND_INIT = (0.03, -0.02, 0.004)        # added to the pair's initial guess for the second alignment

# (name, scan size, fixed iterations (0: converged mode), hessian_mode, overlap_grids)
CASES = [(f"n{n}_k{k}", n, k, 0, 1) for n in SIZES for k in (1, 2, 30, 0)]
CASES += [("n65537_k30_newton", 65537, 30, 1, 1), ("n65537_k30_overlap4", 65537, 30, 0, 4),
          ("n65537_k0_newton", 65537, 0, 1, 1),
          # the 1024-thread instances of the Newton and the overlapping-grids kernels
          ("n300000_k30_newton", 300000, 30, 1, 1), ("n300000_k30_overlap4", 300000, 30, 0, 4),
          ("n4097_k2_newton_overlap4", 4097, 2, 1, 4)]
FIELDS = ("pose", "H", "g", "score", "iterations", "n_hit", "status")


def make_world():
    d = synth.make_pair(2, n_tgt=N_TARGET, n_src=max(SIZES))
    init2 = tuple(a + b for a, b in zip(d["init"], SECOND_INIT))
    return {"tx": d["tx"], "ty": d["ty"], "sx": d["sx"], "sy": d["sy"], "inits": (d["init"], init2)}


def pack(results):
    """AlignResults -> {field: array over the results}, the layout of the fixture."""
    return {"pose": np.array([r.pose for r in results], dtype=np.float64),
            "H": np.array([r.H for r in results], dtype=np.float64),
            "g": np.array([r.g for r in results], dtype=np.float64),
            "score": np.array([r.score for r in results], dtype=np.float64),
            "iterations": np.array([r.iterations for r in results], dtype=np.int32),
            "n_hit": np.array([r.n_hit for r in results], dtype=np.int32),
            "status": np.array([r.status for r in results], dtype=np.int32)}


def run_case(world, dev_scan, case):
    """The case's alignments on one fresh handle: two synchronous ones and, in fixed-iteration mode, the result of two
    asynchronous ones (the last call's, from the second chain).  dev_scan: the whole scan on the device."""
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    _, n, k, mode, overlap = case
    sx, sy = dev_scan[0][:n], dev_scan[1][:n]
    a, b = world["inits"]
    with NdtMatcher2D(fixed_iterations=k, hessian_mode=mode, overlap_grids=overlap) as m:
        m.set_target(world["tx"], world["ty"])
        out = [m.align(sx, sy, a), m.align(sx, sy, b)]
        if k > 0:
            m.align_async(sx, sy, a, producer_complete=True)
            m.align_async(sx, sy, b, producer_complete=True)
            out.append(m.finish())
    return pack(out)
