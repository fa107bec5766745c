"""Timing of the exhaustive pose search for map-to-map alignment (ndt2d_search_map*), host call to host result.

  scans_1k     the config-1 pair as two maps; window +-1 m x +-1 m x full turn at 0.1 m / 2 deg
  room50_20k   the 20k-point config-2 pair; the loop-closure window of the tests: +-2 m x +-2 m x full turn at 0.25 m / 4 deg
               around a guess (1.1, -0.9, 0.35) off the generating pose
  submaps_1M   two config-3-sized submaps (quick_d2d.submap_pair: 1M points each); +-2 m x +-2 m x full turn at 0.1 m / 1 deg

Per case: components, lattice poses, medians of search_map_scores / search_map (k = 8) / search_align_map (k = 8), the
component-pose rate of the volume call, and where the best converged refinement ends.  Prints one JSON line.  Run it
under `rocprofv3 --kernel-trace --stats` (with --profile: fewer repetitions) for per-kernel times."""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gtsam_ndt_amd import search, synth                 # noqa: E402
from gtsam_ndt_amd.matcher import NdtMatcher2D          # noqa: E402
from quick_d2d import med_ms, submap_pair               # noqa: E402

DEG = math.pi / 180.0


def case(tx, ty, sx, sy, window, true_pose, reps):
    res = {}
    with NdtMatcher2D() as t, NdtMatcher2D() as s:
        t.set_target(tx, ty)
        s.set_target(sx, sy)
        out = t.search_align_map(s, *window, k=8)          # first call: builds the derived data and the scratch
        (nt, ny, nx), _ = search.dims(window)
        res["components"] = int(s.components()[0].size)
        res["target_cells"] = int(t.grid_info().n_valid)
        res["lattice"] = [nt, ny, nx]
        res["poses"] = nt * ny * nx
        res["search_map_scores_ms"] = med_ms(lambda: t.search_map_scores(s, *window), reps)
        res["search_map_ms"] = med_ms(lambda: t.search_map(s, *window, k=8), reps)
        res["search_align_map_ms"] = med_ms(lambda: t.search_align_map(s, *window, k=8), reps)
        res["align_map_ms"] = med_ms(lambda: t.align_map(s, out[0][0].pose), reps)
        res["component_poses_per_s_host"] = res["components"] * res["poses"] / (res["search_map_scores_ms"] * 1e-3)
        res["hits"] = len(out)
        conv = [(h, r) for h, r in out if r.converged]
        if conv:
            h, r = max(conv, key=lambda hr: hr[1].score)
            res["best_hit"], res["best_pose"], res["iterations"] = list(h.pose), list(r.pose), r.iterations
            res["best_minus_true"] = [r.pose[0] - true_pose[0], r.pose[1] - true_pose[1],
                                      float(search.wrap(r.pose[2] - true_pose[2]))]
    return res


def main():
    reps = 5 if "--profile" in sys.argv else 25
    out = {}
    d1 = synth.make_pair(1)
    out["scans_1k"] = case(d1["tx"], d1["ty"], d1["sx"], d1["sy"],
                           search.Window(d1["init"], (1.0, 1.0, math.pi), (0.1, 0.1, 2.0 * DEG)), d1["pose"], reps)
    d2 = synth.make_pair(2, n_tgt=20_000, n_src=20_000)
    guess = (d2["pose"][0] + 1.1, d2["pose"][1] - 0.9, d2["pose"][2] + 0.35)
    out["room50_20k"] = case(d2["tx"], d2["ty"], d2["sx"], d2["sy"],
                             search.Window(guess, (2.0, 2.0, math.pi), (0.25, 0.25, 4.0 * DEG)), d2["pose"], reps)
    d3, mx, my = submap_pair()
    guess = (d3["pose"][0] + 1.1, d3["pose"][1] - 0.9, d3["pose"][2] + 0.35)
    out["submaps_1M"] = case(d3["tx"], d3["ty"], mx, my,
                             search.Window(guess, (2.0, 2.0, math.pi), (0.1, 0.1, 1.0 * DEG)), d3["pose"], reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
