"""Timing of 3D map-to-map alignment (ndt3d_align_map) next to the point-to-map path it shares its launch chain with.

  maps_1m            the config-5 pair as two 1 m voxel maps, from a start 5 cm / 5 mrad off the generating pose
  maps_1m_zero       maps_1m from the zero guess: the local optimum 0.3 m off with the own voxel alone, the
                     generating pose with --map-neighbourhood 7
  maps_2m            the same clouds at 2 m voxels, from the zero guess
  coarse_then_fine   maps_2m from the zero guess, then maps_1m from its result: how a caller gets past the local optimum
  point_to_map       ndt3d_align_dev of the config-5 scan against the 1 m grid (the existing path)

Per map case: components, host-call-to-result time of a converged alignment, time per launch of the chain from two
fixed-iteration runs ((t(K2) - t(K1)) / (K2 - K1)), the one-off cost of the derived data (first call after a grid change
minus a later one) and the distance of the result to the generating pose.  --map-neighbourhood 7: every target of the map cases
scores a component against its own voxel and the six face neighbours (ndt3d_set_map_neighbourhood; default 1).
Prints one JSON line.  Run it under
`rocprofv3 --kernel-trace --stats` (with --profile: fewer repetitions) for per-kernel times."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_ndt_amd import synth3d                    # noqa: E402
from gtsam_ndt_amd.matcher import NdtMatcher3D       # noqa: E402


def med_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def per_launch_us(make, run, reps, k1=20, k2=120):
    out = []
    for k in (k1, k2):
        h = make(k)
        run(h)
        out.append(med_ms(lambda: run(h), reps))
    return (out[1] - out[0]) * 1e3 / (k2 - k1)


MAP_NB = int(sys.argv[sys.argv.index("--map-neighbourhood") + 1]) if "--map-neighbourhood" in sys.argv else 1


def pair_of_maps(d, cell, **kw):
    t, s = NdtMatcher3D(cell_size=cell, map_neighbourhood=MAP_NB, **kw), NdtMatcher3D(cell_size=cell)
    t.set_target(d["tx"], d["ty"], d["tz"])
    s.set_target(d["sx"], d["sy"], d["sz"])
    return t, s


def off_truth(pose, d):
    e = np.abs(np.array(pose) - np.array(d["pose"]))
    return [float(e[:3].max()), float(e[3:].max())]


def map_case(d, cell, init, reps):
    res = {}
    t, s = pair_of_maps(d, cell)
    t0 = time.perf_counter()
    r = t.align_map(s, init)
    first = (time.perf_counter() - t0) * 1e3
    res["components"] = int(s.components()[0].size)
    res["target_voxels"] = int(t.grid_info().n_valid)
    res["align_map_ms"] = med_ms(lambda: t.align_map(s, init), reps)
    res["first_call_extra_ms"] = first - res["align_map_ms"]
    res["iterations"], res["status"], res["n_hit"] = r.iterations, r.status, r.n_hit
    res["pose"] = list(r.pose)
    res["off_generating_pose_m_rad"] = off_truth(r.pose, d)
    res["evaluate_map_ms"] = med_ms(lambda: t.evaluate_map(s, init), reps)
    t.close(); s.close()
    for name, mode in (("us_per_launch", 0), ("us_per_launch_newton", 1)):
        res[name] = per_launch_us(lambda k: pair_of_maps(d, cell, fixed_iterations=k, hessian_mode=mode),
                                  lambda h: h[0].align_map(h[1], init), reps)
    return res


def main():
    import torch
    reps = 5 if "--profile" in sys.argv else 25
    d = synth3d.make_pair3d()
    zero = (0.0,) * 6
    near = tuple(np.array(d["pose"]) + np.array([0.05, -0.05, 0.02, 0.005, -0.005, 0.005]))
    out = {"true_pose": list(d["pose"]), "map_neighbourhood": MAP_NB}
    out["maps_1m"] = map_case(d, 1.0, near, reps)
    out["maps_1m_zero"] = map_case(d, 1.0, zero, reps)
    out["maps_2m"] = map_case(d, 2.0, zero, reps)
    t2, s2 = pair_of_maps(d, 2.0)
    t1, s1 = pair_of_maps(d, 1.0)
    direct = t1.align_map(s1, zero)

    def two_step():
        c = t2.align_map(s2, zero)
        return c, t1.align_map(s1, c.pose)
    c, f = two_step()
    out["coarse_then_fine"] = {"iterations": [c.iterations, f.iterations], "status": [c.status, f.status],
                               "off_generating_pose_m_rad": off_truth(f.pose, d), "ms": med_ms(two_step, reps),
                               "direct_1m_from_zero_off_generating_pose_m_rad": off_truth(direct.pose, d),
                               "direct_1m_from_zero_iterations": direct.iterations}
    sx, sy, sz = (torch.from_numpy(d["s" + a]).cuda() for a in "xyz")
    torch.cuda.synchronize()

    def make(k):
        h = NdtMatcher3D(fixed_iterations=k)
        h.set_target(d["tx"], d["ty"], d["tz"])
        return h
    out["point_to_map"] = {"us_per_launch": per_launch_us(make, lambda h: h.align(sx, sy, sz, zero), reps)}
    h = make(0)
    r = h.align(sx, sy, sz, zero)
    out["point_to_map"].update(align_dev_ms=med_ms(lambda: h.align(sx, sy, sz, zero), reps), iterations=r.iterations,
                               off_generating_pose_m_rad=off_truth(r.pose, d))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
