"""The alignments of tests/test_gpu_packed_partials.py and of tests/golden/make_packed_partials_golden.py, which
records what they return (tests/golden/packed_partials.npz).  One definition, so that the fixture and the test cannot
drift apart.

What they are for: the single-scan chain hands a launch's sums to the next as three 16-byte entries per workgroup
(AlignDyn::partials, float4[2][3][256]) instead of twelve floats in twelve rows, and three waves fold four sums each
instead of four waves three.  Every sum is formed from the same operands in the same order, so every result must be,
bit for bit, what the row-per-sum table gave.  The cases go through every instance of k_iterate / k_iterate_first
(Gauss-Newton and Newton, one and four grids, 256 and 1024 threads), every way a chain is driven (synchronous, 1 to 4
asynchronous calls on one and on two launch chains, converged mode in chunks of 2 and 8, plain launches, k_begin in
front, K = 1, line search, an alignment that ends at its first solve), every row of ndt2d_align_trace and
ndt2d_evaluate_dev.

The world is tests/first_launch_cases.py's (a 20 000-point target, scans of 4 097 to 6 000 points: the smallest at
which these kernels run).  With 4 097 points and 256-thread workgroups, 239 of the 256 workgroups have no point (with
1024-thread workgroups, 251): their entries of the table must be written as zeros and folded.

A case is (name, matcher parameters, tuning knobs, steps); a step is one of first_launch_cases' two
    ("sync", scan, init)            one synchronous alignment                       -> one result
    ("async", (scan, init), ...)    that many asynchronous calls, then finish       -> the last call's result
or
    ("trace", scan, init)           ndt2d_align_trace                               -> one result per row
    ("eval", scan, pose)            ndt2d_evaluate_dev at `pose`                    -> one result (pose as given,
                                                                                       iterations = status = 0)
All steps of a case run on one handle, in order."""
import numpy as np

import first_launch_cases as fc

FIELDS = fc.FIELDS
make_world = fc.make_world
to_device = fc.to_device
open_matcher = fc.open_matcher
I0, I1, I2, NEAR, FAR, POOR = fc.I0, fc.I1, fc.I2, fc.NEAR, fc.FAR, fc.POOR

_FOUR = (("s6000", I0), ("s4097", I1), ("s5000", I2), ("s6000", I1))
_ASYNC_1_TO_4 = [("async",) + _FOUR[:n] for n in (1, 2, 3, 4)]
_WIDE = {"wide_threshold": 4097}          # every scan here runs the 1024-thread instances

CASES = [
    # the four 256-thread instances, synchronous; the 4 097-point scan leaves most workgroups without points
    ("gn_k3", dict(fixed_iterations=3), {}, [("sync", "s4097", I0), ("sync", "s6000", I1), ("sync", "s5000", I2)]),
    ("newton_k3", dict(fixed_iterations=3, hessian_mode=1), {}, [("sync", "s4097", I0), ("sync", "s6000", I1)]),
    ("gn_overlap4_k3", dict(fixed_iterations=3, overlap_grids=4), {}, [("sync", "s4097", I0), ("sync", "s6000", I1)]),
    ("newton_overlap4_k3", dict(fixed_iterations=3, hessian_mode=1, overlap_grids=4), {}, [("sync", "s4097", I0),
                                                                                           ("sync", "s5000", I2)]),
    # the four 1024-thread instances (16 waves: three fold, thirteen stand by)
    ("wide_gn_k3", dict(fixed_iterations=3), _WIDE, [("sync", "s4097", I0), ("sync", "s6000", I1)] + _ASYNC_1_TO_4[1:2]),
    ("wide_newton_k3", dict(fixed_iterations=3, hessian_mode=1), _WIDE, [("sync", "s4097", I0), ("sync", "s6000", I1)]),
    ("wide_gn_overlap4_k3", dict(fixed_iterations=3, overlap_grids=4), _WIDE, [("sync", "s4097", I0), ("sync", "s5000", I2)]),
    ("wide_newton_overlap4_k3", dict(fixed_iterations=3, hessian_mode=1, overlap_grids=4), _WIDE,
     [("sync", "s4097", I0), ("sync", "s6000", I1)]),
    ("wide_converged", dict(), _WIDE, [("sync", "s4097", NEAR), ("sync", "s6000", FAR)]),
    # 1 to 4 asynchronous calls, on one launch chain and on two (each chain has a table of its own)
    ("async_one_lane", dict(fixed_iterations=3), {"async_lanes": 1}, _ASYNC_1_TO_4),
    ("async_two_lanes", dict(fixed_iterations=3), {"async_lanes": 2}, _ASYNC_1_TO_4),
    ("async_two_lanes_newton_overlap4", dict(fixed_iterations=2, hessian_mode=1, overlap_grids=4), {"async_lanes": 2},
     _ASYNC_1_TO_4[1:]),
    # converged mode, chunks of 2 and 8
    ("converged_chunk2", dict(), {"chunk_launches": 2}, [("sync", "s4097", NEAR), ("sync", "s6000", FAR),
                                                          ("async", ("s5000", FAR), ("s4097", NEAR))]),
    ("converged_chunk8", dict(), {"chunk_launches": 8}, [("sync", "s4097", NEAR), ("sync", "s6000", FAR),
                                                          ("async", ("s5000", FAR), ("s4097", NEAR))]),
    # plain launches instead of graph replays
    ("no_graph_k3", dict(fixed_iterations=3), {"launch_graphs": 0}, [("sync", "s4097", I0), ("async",) + _FOUR[:2]]),
    ("no_graph_converged", dict(), {"launch_graphs": 0, "chunk_launches": 4}, [("sync", "s6000", FAR), ("sync", "s4097", NEAR)]),
    # k_begin in front of K + 1 k_iterate launches: launch 0 is a k_iterate, not a k_iterate_first
    ("k_begin_k3", dict(fixed_iterations=3), {"fused_begin": 0}, [("sync", "s4097", I0), ("sync", "s6000", I1),
                                                                  ("async",) + _FOUR[:3]]),
    ("k_begin_converged", dict(), {"fused_begin": 0}, [("sync", "s4097", NEAR), ("sync", "s5000", FAR)]),
    # K = 1: one launch reads the table the first launch wrote
    ("k1", dict(fixed_iterations=1), {}, [("sync", "s4097", I0), ("sync", "s6000", I1), ("async",) + _FOUR[:2]]),
    # line search
    ("line_search_k6", dict(fixed_iterations=6, line_search=4), {}, [("sync", "s6000", POOR), ("sync", "s4097", I0)]),
    ("line_search_converged", dict(line_search=4), {}, [("sync", "s6000", POOR), ("sync", "s4097", POOR)]),
    # an alignment that ends at its first solve (n_hit < min_hits), the remaining launches carry the state
    ("too_few_hits", dict(fixed_iterations=4), {}, [("sync", "off_grid", I0), ("sync", "s4097", I0),
                                                    ("async", ("off_grid", I0), ("s5000", I1))]),
    ("too_few_hits_converged", dict(), {}, [("sync", "off_grid", I0), ("sync", "s4097", I0)]),
    # ndt2d_align_trace, every row; an alignment before and after it on the same handle
    ("trace_k6", dict(fixed_iterations=6), {}, [("sync", "s6000", I1), ("trace", "s4097", I0), ("trace", "s6000", FAR),
                                                 ("sync", "s5000", I2)]),
    ("trace_converged", dict(), {}, [("trace", "s4097", FAR), ("trace", "s6000", NEAR)]),
    ("trace_wide_newton_overlap4", dict(fixed_iterations=4, hessian_mode=1, overlap_grids=4), _WIDE, [("trace", "s4097", I0)]),
    ("trace_line_search", dict(fixed_iterations=6, line_search=4), {}, [("trace", "s6000", POOR)]),
    # ndt2d_evaluate_dev
    ("eval", dict(), {}, [("eval", "s4097", I0), ("eval", "s6000", fc.NEAR), ("sync", "s5000", I0), ("eval", "s5000", I2),
                          ("eval", "off_grid", I0)]),
    ("eval_wide_newton_overlap4", dict(hessian_mode=1, overlap_grids=4), _WIDE, [("eval", "s4097", I0), ("eval", "s6000", I1)]),
]
CASE_IDS = [c[0] for c in CASES]


def _eval_fields(ev, pose):
    H, g, score, n_hit = ev
    return {"pose": np.array([pose], dtype=np.float64), "H": H[None], "g": g[None], "score": np.array([score], dtype=np.float64),
            "iterations": np.zeros(1, dtype=np.int32), "n_hit": np.array([n_hit], dtype=np.int32),
            "status": np.zeros(1, dtype=np.int32)}


def run_case(world, dev, case):
    """The case's steps on one fresh handle -> {field: array over all results of all steps}."""
    parts = []
    with open_matcher(world, case, None) as m:
        for step in case[3]:
            if step[0] == "sync":
                parts.append(fc.pack([m.align(*dev[step[1]], step[2])]))
            elif step[0] == "async":
                for scan, init in step[1:]:
                    m.align_async(*dev[scan], init, producer_complete=True)
                parts.append(fc.pack([m.finish()]))
            elif step[0] == "trace":
                rows = m.align_trace(*world["scans"][step[1]], step[2])
                assert rows
                parts.append(fc.pack(rows))
            else:
                parts.append(_eval_fields(m.evaluate(*dev[step[1]], step[2]), step[2]))
    return {f: np.concatenate([p[f] for p in parts]) for f in FIELDS}
