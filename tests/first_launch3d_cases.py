"""The 3D twin of tests/first_launch_cases.py: the alignments of tests/test_gpu_first_launch3d.py and of
tests/golden/make_first_launch_golden.py, which records what they return (tests/golden/first_launch3d.npz).

The first launch of a 3D chain carries the call's arguments itself (k_iterate3_first) instead of following a k_begin3.
The world is the smallest config-5-style pair the 3D tests use, make_pair3d(16, 256): 4 096 points either side, and a
3 000-point prefix of the scan in buffers of its own.  K <= 4; fixed and converged mode; at least two calls per handle.
Cases, steps and `fused` as in first_launch_cases.py."""
import numpy as np

from gtsam_ndt_amd import synth3d

FIELDS = ("pose", "H", "g", "score", "iterations", "n_hit", "status")
NDT_TOO_FEW_HITS = 3

I0 = (0.0,) * 6
I1 = (0.05, -0.04, 0.02, 0.002, -0.003, 0.005)
I2 = (-0.06, 0.03, -0.01, -0.004, 0.002, -0.006)
TWO_PI = 6.283185307179586
TURNED = (0.05, -0.04, 0.02, 0.002 + TWO_PI, -0.003 - TWO_PI, 0.005 + TWO_PI)      # I1, every angle a whole turn off

CASES = [
    ("k3", dict(fixed_iterations=3), {}, [("sync", "full", I0), ("sync", "part", I1), ("sync", "full", I2),
                                          ("async", ("part", I2), ("full", I1))]),
    ("k1", dict(fixed_iterations=1), {}, [("sync", "full", I0), ("sync", "part", I1)]),
    ("k4_newton", dict(fixed_iterations=4, hessian_mode=1), {}, [("sync", "full", I0), ("sync", "part", I1)]),
    ("converged", dict(), {}, [("sync", "full", I0), ("sync", "part", I1), ("async", ("full", I2))]),
    ("converged_newton", dict(hessian_mode=1), {}, [("sync", "part", I0), ("sync", "full", I1)]),
    # initial angles outside (-pi, pi]: wrap_angle in every thread of launch 0
    ("angles_wrap_k2", dict(fixed_iterations=2), {}, [("sync", "full", TURNED), ("sync", "full", (0.0, 0.0, 0.0, 0.0, 0.0, 3.5)),
                                                      ("sync", "part", (0.0, 0.0, 0.0, 0.0, 0.0, -7.0))]),
    # line search: both slots are reset by the first launch
    ("line_search_converged", dict(line_search=3), {}, [("sync", "full", I0), ("sync", "full", I0)]),
    # an alignment that ends at its first solve (a scan off the grid), then a normal one
    ("too_few_hits_k2", dict(fixed_iterations=2), {}, [("sync", "off_grid", I0), ("sync", "full", I0)]),
    ("too_few_hits_converged", dict(), {}, [("sync", "off_grid", I0), ("sync", "part", I0)]),
]
CASE_IDS = [c[0] for c in CASES]


def n_results(case):
    return len(case[3])


def is_fixed(case):
    return case[1].get("fixed_iterations", 0) > 0


def make_world():
    d = synth3d.make_pair3d(16, 256)
    c = np.ascontiguousarray
    full = (d["sx"], d["sy"], d["sz"])
    scans = {"full": full, "part": tuple(c(a[:3000]) for a in full),
             "off_grid": (c(full[0] + np.float32(1000.0)), full[1], full[2])}
    return {"t": (d["tx"], d["ty"], d["tz"]), "scans": scans}


def to_device(world):
    """Every scan in device buffers of its own."""
    import torch
    dev = {k: tuple(torch.from_numpy(a).cuda() for a in v) for k, v in world["scans"].items()}
    torch.cuda.synchronize()
    return dev


def pack(results):
    return {"pose": np.array([r.pose for r in results], dtype=np.float64),
            "H": np.array([r.H for r in results], dtype=np.float64),
            "g": np.array([r.g for r in results], dtype=np.float64),
            "score": np.array([r.score for r in results], dtype=np.float64),
            "iterations": np.array([r.iterations for r in results], dtype=np.int32),
            "n_hit": np.array([r.n_hit for r in results], dtype=np.int32),
            "status": np.array([r.status for r in results], dtype=np.int32)}


def open_matcher(world, case, fused):
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    tuning = dict(case[2])
    if fused is not None:
        tuning["fused_begin"] = fused
    m = NdtMatcher3D(tuning=tuning, **case[1])
    m.set_target(*world["t"])
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
    """The last row of ndt3d_align_trace - k_begin3 and K + 1 plain launches, whatever the knob says - for every
    synchronous step of a fixed-iteration case, on one handle: {step index: result}."""
    out = {}
    with open_matcher(world, case, fused) as m:
        for j, step in enumerate(case[3]):
            if step[0] == "sync":
                out[j] = m.align_trace(*world["scans"][step[1]], step[2])[-1]
    return out
