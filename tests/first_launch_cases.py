"""The alignments of tests/test_gpu_first_launch.py and of tests/golden/make_first_launch_golden.py, which records what
they return (tests/golden/first_launch.npz).  One definition, so that the fixture and the test cannot drift apart.

What they are for: the first launch of a single-scan chain carries the call's arguments itself (k_iterate_first) instead
of following a k_begin.  tests/chain_head_cases.py already runs that path at 1, 2 and 30 iterations; the cases here are
the ways such a fused launch can go wrong that those do not reach (a launch >= 1 reading the previous call's n or
pointers, an unwrapped initial angle, line-search state surviving a call, an alignment that ends at its first solve,
the chunk bookkeeping of converged mode with launch 0 outside the chunks, plain launches, a graph of one launch).

The world is the smallest at which these kernels run: the 20 000-point target of make_pair(2, n_tgt=20000) and scans of
4 097 to 6 000 points cut from one 6 000-point scan of it (the generator emits points in random order, so any slice is a
scan of its own): k_align_small ends at 4 096 points.  Fixed-iteration cases use K <= 6.

A case is (name, matcher parameters, tuning knobs, steps); a step is
    ("sync", scan, init)            one synchronous alignment                                   -> one result
    ("async", (scan, init), ...)    that many asynchronous calls, then finish                   -> the last call's result
All steps of a case run on one handle, in order.  `fused`: None leaves NDT_TUNE_FUSED_BEGIN alone (the recording is
taken from a library that does not know the knob), 0 / 1 sets it."""
import numpy as np

from gtsam_ndt_amd import synth

N_TARGET = 20_000
N_SCAN = 6_000
FIELDS = ("pose", "H", "g", "score", "iterations", "n_hit", "status")
NDT_TOO_FEW_HITS = 3

# initial poses: the pair's guess (0, 0, 0; the scan was taken at T_STAR = (0.10, -0.08, 0.01)) and others around it
I0 = (0.0, 0.0, 0.0)
I1 = (0.03, -0.02, 0.004)
I2 = (-0.05, 0.04, -0.01)
NEAR = (0.099, -0.079, 0.0099)      # converges in few iterations
FAR = (0.55, -0.45, 0.09)           # ... in many
POOR = (0.45, 0.35, -0.08)          # far enough for line-search steps that score worse
TWO_PI = 6.283185307179586

_STALE = (("s6000", I0), ("s4097", I1), ("s5000", I2), ("s6000", I1))

CASES = [
    # 1. stale per-call arguments: three scans of different sizes in different buffers, different poses, one handle
    ("stale_sync", dict(fixed_iterations=3), {}, [("sync", s, i) for s, i in _STALE[:3]]),
    ("stale_async", dict(fixed_iterations=3), {}, [("async",) + _STALE[:n] for n in (1, 2, 3, 4)]),
    # 2. initial yaw outside (-pi, pi]: wrap_angle in every thread of launch 0 (3.5 and -7.0 rad, and a good guess a
    # whole turn off either way)
    ("yaw_wrap", dict(fixed_iterations=3), {}, [("sync", "s5000", (0.0, 0.0, 3.5)), ("sync", "s5000", (0.0, 0.0, -7.0)),
                                                 ("sync", "s6000", (0.03, -0.02, 0.01 + TWO_PI)),
                                                 ("sync", "s6000", (0.03, -0.02, 0.01 - TWO_PI))]),
    ("yaw_wrap_converged", dict(), {}, [("sync", "s5000", (0.0, 0.0, 0.004 + TWO_PI)), ("sync", "s5000", (0.0, 0.0, -7.0))]),
    # 3. line search: ls[] is reset by the first launch, so the second alignment starts clean
    ("line_search_k6", dict(fixed_iterations=6, line_search=4), {}, [("sync", "s6000", POOR), ("sync", "s6000", POOR),
                                                                     ("sync", "s4097", I0)]),
    ("line_search_converged", dict(line_search=4), {}, [("sync", "s6000", POOR), ("sync", "s6000", POOR)]),
    # 4. an alignment that ends at its first solve (a scan off the grid: NDT_TOO_FEW_HITS), the remaining launches carry
    # the state; then a normal one on the same handle
    ("too_few_hits_fixed", dict(fixed_iterations=4), {}, [("sync", "off_grid", I0), ("sync", "s5000", I0),
                                                          ("async", ("off_grid", I0), ("s5000", I1))]),
    ("too_few_hits_converged", dict(), {}, [("sync", "off_grid", I0), ("sync", "s5000", I0)]),
    # 5. converged mode: launch 0 is outside the chunks; few and many iterations; a second call straight after
    ("converged_chunk2", dict(), {"chunk_launches": 2}, [("sync", "s6000", NEAR), ("sync", "s6000", FAR),
                                                          ("sync", "s4097", NEAR), ("async", ("s5000", FAR))]),
    ("converged_chunk8", dict(), {"chunk_launches": 8}, [("sync", "s6000", NEAR), ("sync", "s6000", FAR),
                                                          ("sync", "s4097", NEAR), ("async", ("s5000", FAR))]),
    # 6. plain launches instead of graph replays
    ("no_graph_k3", dict(fixed_iterations=3), {"launch_graphs": 0}, [("sync", "s6000", I0), ("sync", "s4097", I1),
                                                                      ("async", ("s5000", I2))]),
    ("no_graph_converged", dict(), {"launch_graphs": 0, "chunk_launches": 4}, [("sync", "s6000", FAR), ("sync", "s5000", NEAR)]),
    # 7. K = 1: a graph of one launch, starting at parity 1
    ("k1", dict(fixed_iterations=1), {}, [("sync", "s6000", I0), ("sync", "s4097", I1),
                                          ("async", ("s5000", I2), ("s6000", I1))]),
    # the other instances of the first-launch kernel: 1024-thread workgroups (wide_threshold lowered to 6 000),
    # Newton Hessian, four overlapping grids
    ("wide_k3", dict(fixed_iterations=3), {"wide_threshold": 6000}, [("sync", "s6000", I0), ("sync", "s5000", I1),
                                                                      ("async", ("s6000", I2), ("s6000", I1))]),
    ("wide_newton_overlap4_k2", dict(fixed_iterations=2, hessian_mode=1, overlap_grids=4), {"wide_threshold": 6000},
     [("sync", "s6000", I0), ("sync", "s6000", I1)]),
    ("newton_overlap4_k2", dict(fixed_iterations=2, hessian_mode=1, overlap_grids=4), {}, [("sync", "s5000", I0),
                                                                                          ("sync", "s4097", I1)]),
    ("newton_k2", dict(fixed_iterations=2, hessian_mode=1), {}, [("sync", "s5000", I0)]),
    ("overlap4_converged", dict(overlap_grids=4), {}, [("sync", "s5000", I0), ("sync", "s6000", I1)]),
]
CASE_IDS = [c[0] for c in CASES]


def n_results(case):
    return len(case[3])


def is_fixed(case):
    return case[1].get("fixed_iterations", 0) > 0


def make_world():
    d = synth.make_pair(2, n_tgt=N_TARGET, n_src=N_SCAN)
    sx, sy = d["sx"], d["sy"]
    c = np.ascontiguousarray
    scans = {"s6000": (sx, sy), "s4097": (c(sx[:4097]), c(sy[:4097])), "s5000": (c(sx[1000:]), c(sy[1000:])),
             # translated off the grid: no point lands in a cell
             "off_grid": (c(sx[1000:] + np.float32(1000.0)), c(sy[1000:]))}
    assert [scans[k][0].size for k in ("s6000", "s4097", "s5000", "off_grid")] == [6000, 4097, 5000, 5000]
    return {"tx": d["tx"], "ty": d["ty"], "scans": scans}


def to_device(world):
    """Every scan in device buffers of its own."""
    import torch
    dev = {k: (torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()) for k, (x, y) in world["scans"].items()}
    torch.cuda.synchronize()
    return dev


def pack(results):
    """AlignResults -> {field: array over the results}, the layout of the fixture."""
    return {"pose": np.array([r.pose for r in results], dtype=np.float64),
            "H": np.array([r.H for r in results], dtype=np.float64),
            "g": np.array([r.g for r in results], dtype=np.float64),
            "score": np.array([r.score for r in results], dtype=np.float64),
            "iterations": np.array([r.iterations for r in results], dtype=np.int32),
            "n_hit": np.array([r.n_hit for r in results], dtype=np.int32),
            "status": np.array([r.status for r in results], dtype=np.int32)}


def open_matcher(world, case, fused):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    tuning = dict(case[2])
    if fused is not None:
        tuning["fused_begin"] = fused
    m = NdtMatcher2D(tuning=tuning, **case[1])
    m.set_target(world["tx"], world["ty"])
    return m


def run_case(world, dev, case, fused=None):
    """The case's steps on one fresh handle, one result per step."""
    out = []
    with open_matcher(world, case, fused) as m:
        for step in case[3]:
            if step[0] == "sync":
                out.append(m.align(*dev[step[1]], step[2]))
            else:
                for scan, init in step[1:]:
                    m.align_async(*dev[scan], init, producer_complete=True)
                out.append(m.finish())
    return pack(out)


def run_trace(world, case, fused=None):
    """The last row of ndt2d_align_trace - k_begin and K + 1 plain launches, whatever the knob says - for every
    synchronous step of a fixed-iteration case, on one handle: {step index: result}."""
    out = {}
    with open_matcher(world, case, fused) as m:
        for j, step in enumerate(case[3]):
            if step[0] == "sync":
                out[j] = m.align_trace(*world["scans"][step[1]], step[2])[-1]
    return out
