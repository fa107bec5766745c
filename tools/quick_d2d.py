"""Timing of map-to-map alignment (ndt2d_align_map) next to the point-to-map path it shares its launch chain with.

  submaps_1M         two config-3-sized submaps (the 4x4-room scene, 1M points each, independent samplings a known pose apart)
  scans_1k           two maps of one config-1 scan each
  point_to_map_100k  ndt2d_align_dev of the 100k-point config-3 scan against the 1M-point submap (the existing path)

Per map case: components, host-call-to-result time of a converged alignment, time per launch of the chain from two
fixed-iteration runs ((t(K2) - t(K1)) / (K2 - K1)), the one-off cost of the derived data (first call after a grid change
minus a later one) and how the map-to-map pose differs from the point-to-map pose of the same scene.  Prints one JSON
line.  Run it under `rocprofv3 --kernel-trace --stats` (with --profile: fewer repetitions) for per-kernel times."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_ndt_amd import synth                      # noqa: E402
from gtsam_ndt_amd.matcher import NdtMatcher2D       # noqa: E402


def submap_pair():
    """The config-3 submap and a second 1M-point sampling of the same 16 rooms, in a frame T_STAR off room (2,1)'s centre."""
    d = synth.make_pair(3)
    L, S, tiles = 50.0, 3, 4
    half = 0.5 * tiles * L
    scene = None
    for j in range(tiles):
        for i in range(tiles):
            r = synth.room_scene(S + 1000 * (j * tiles + i), L, i * L - half, j * L - half)
            scene = r if scene is None else scene.concat(r)
    xs, ys = synth.sample_scene(scene, 1_000_000, seed=S * 7919 + 13, sigma=synth.SIGMA)
    xs, ys = synth.to_source_frame(xs, ys, d["pose"])
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)
    return d, f(xs), f(ys)


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


def map_case(tx, ty, sx, sy, init, reps):
    res = {}
    with NdtMatcher2D() as t, NdtMatcher2D() as s:
        t.set_target(tx, ty)
        s.set_target(sx, sy)
        t0 = time.perf_counter()
        r = t.align_map(s, init)
        first = (time.perf_counter() - t0) * 1e3
        res["components"] = int(s.components()[0].size)
        res["target_cells"] = int(t.grid_info().n_valid)
        res["align_map_ms"] = med_ms(lambda: t.align_map(s, init), reps)
        res["first_call_extra_ms"] = first - res["align_map_ms"]
        res["iterations"], res["status"], res["n_hit"] = r.iterations, r.status, r.n_hit
        res["pose"] = list(r.pose)
        res["evaluate_map_ms"] = med_ms(lambda: t.evaluate_map(s, init), reps)
        p2m = t.align(sx, sy, init)
        res["point_to_map_pose"] = list(p2m.pose)
        res["pose_minus_point_to_map"] = [a - b for a, b in zip(r.pose, p2m.pose)]

    def make(k):
        a, b = NdtMatcher2D(fixed_iterations=k), NdtMatcher2D()
        a.set_target(tx, ty)
        b.set_target(sx, sy)
        return a, b
    res["us_per_launch"] = per_launch_us(make, lambda h: h[0].align_map(h[1], init), reps)
    return res


def main():
    import torch
    reps = 5 if "--profile" in sys.argv else 25
    out = {}
    d3, mx, my = submap_pair()
    out["submaps_1M"] = map_case(d3["tx"], d3["ty"], mx, my, d3["init"], reps)
    out["submaps_1M"]["true_pose"] = list(d3["pose"])
    d1 = synth.make_pair(1)
    out["scans_1k"] = map_case(d1["tx"], d1["ty"], d1["sx"], d1["sy"], d1["init"], reps)
    out["scans_1k"]["true_pose"] = list(d1["pose"])
    sx, sy = torch.from_numpy(d3["sx"]).cuda(), torch.from_numpy(d3["sy"]).cuda()
    torch.cuda.synchronize()

    def make(k):
        h = NdtMatcher2D(fixed_iterations=k)
        h.set_target(d3["tx"], d3["ty"])
        return h
    out["point_to_map_100k"] = {"us_per_launch": per_launch_us(make, lambda h: h.align(sx, sy, d3["init"]), reps)}
    with NdtMatcher2D() as h:
        h.set_target(d3["tx"], d3["ty"])
        h.align(sx, sy, d3["init"])
        out["point_to_map_100k"]["align_dev_ms"] = med_ms(lambda: h.align(sx, sy, d3["init"]), reps)
        out["point_to_map_100k"]["iterations"] = h.align(sx, sy, d3["init"]).iterations
    print(json.dumps(out))


if __name__ == "__main__":
    main()
