"""Timing of the exhaustive pose search for 3D map-to-map alignment (ndt3d_search_map*), host call to host result.

  half_1m   the 32 x 1024-beam pair (generating pose (2, -1.5, 0.02, 0.004, -0.003, 0.6)) at 1 m voxels; the loop-closure
            window of the tests: +-3 m x +-3 m x full turn at 0.5 m / 4 deg around a guess (1.6, -1.3, 0.5 rad) off that pose
  full_1m   the full config-5 pair (64 x 2048 beams, the same pose) at 1 m voxels; +-3 m x +-3 m x full turn at 0.25 m / 2 deg
  full_05m  the same clouds at 0.5 m voxels; +-3 m x +-3 m x full turn at 0.25 m / 2 deg

Per case: components, lattice poses, medians of search_map_scores / search_map (k = 8) / search_align_map (k = 8), the
component-pose rate of the volume call, and where the best converged refinement ends.  Prints one JSON line.  Run it
under `rocprofv3 --kernel-trace --stats` with the program after `--` (with --profile: fewer repetitions) for per-kernel
times."""
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gtsam_ndt_amd import search, synth3d               # noqa: E402
from quick_d2d3 import med_ms, pair_of_maps             # noqa: E402

DEG = math.pi / 180.0
POSE = (2.0, -1.5, 0.02, 0.004, -0.003, 0.6)
OFFSET = (1.6, -1.3, 0.0, 0.0, 0.0, 0.5)


def case(d, cell, window, reps):
    res = {}
    t, s = pair_of_maps(d, cell)
    try:
        out = t.search_align_map(s, *window, k=8)          # first call: builds the derived data and the scratch
        (nt, ny, nx), _ = search.dims(window)
        res["components"] = int(s.components()[0].size)
        res["target_voxels"] = int(t.grid_info().n_valid)
        res["lattice"] = [nt, ny, nx]
        res["poses"] = nt * ny * nx
        res["search_map_scores_ms"] = med_ms(lambda: t.search_map_scores(s, *window), reps)
        res["search_map_ms"] = med_ms(lambda: t.search_map(s, *window, k=8), reps)
        res["search_align_map_ms"] = med_ms(lambda: t.search_align_map(s, *window, k=8), reps)
        res["align_map_ms"] = med_ms(lambda: t.align_map(s, out[0][0].pose), reps)
        res["component_poses_per_s_host"] = res["components"] * res["poses"] / (res["search_map_scores_ms"] * 1e-3)
        res["hits"] = len(out)
        conv = [(h, r) for h, r in out if r.status == 0]          # (AlignResult3D has no .converged)
        if conv:
            h, r = max(conv, key=lambda hr: hr[1].score)
            res["best_hit"], res["best_pose"], res["iterations"] = list(h.pose), list(r.pose), r.iterations
            res["best_minus_true"] = [r.pose[a] - d["pose"][a] for a in range(3)] + \
                                     [float(search.wrap(r.pose[a] - d["pose"][a])) for a in range(3, 6)]
    finally:
        t.close(); s.close()
    return res


def main():
    reps = 5 if "--profile" in sys.argv else 25
    guess = tuple(a + b for a, b in zip(POSE, OFFSET))
    out = {}
    half = synth3d.make_pair3d(n_elev=32, n_azim=1024, pose=POSE)
    out["half_1m"] = case(half, 1.0, search.Window(guess, (3.0, 3.0, math.pi), (0.5, 0.5, 4.0 * DEG)), reps)
    full = synth3d.make_pair3d(pose=POSE)
    fine = search.Window(guess, (3.0, 3.0, math.pi), (0.25, 0.25, 2.0 * DEG))
    out["full_1m"] = case(full, 1.0, fine, reps)
    out["full_05m"] = case(full, 0.5, fine, reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
