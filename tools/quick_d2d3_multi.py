"""Timing of ndt3d_align_map_multi and of ndt3d_search_align_map, which refines its hits through it (a config-5 pair at
1 m voxels, about 2 500 source components, the loop-closure window of tests/test_gpu_search_map3d.py).

  search_map / search_align_map, k = 8 and 64   host-timed; their difference is the refinement of the hits
  align_map_multi, m = 1, 2, 8, 64              starts = the poses of the search's hits
each once with one chain for all starts (NDT_TUNE_MAP_MULTI_FROM = 1, "chain") and once with one ndt3d_align_map chain
per start (65, "loop": what ndt3d_search_align_map did per hit before the chain existed).

Medians (and the range) of 25 calls after a warm-up call; one JSON line.  On a library without ndt3d_align_map_multi
only the search figures are printed (the comparison column).  Under `rocprofv3 --kernel-trace --stats` pass --profile
(5 calls)."""
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_ndt_amd import search, synth3d            # noqa: E402
from gtsam_ndt_amd.matcher import NdtMatcher3D       # noqa: E402

POSE = (2.0, -1.5, 0.02, 0.004, -0.003, 0.6)
OFFSET = (1.6, -1.3, 0.0, 0.0, 0.0, 0.5)


def timed_ms(fn, reps):
    """[median, min, max] in milliseconds"""
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return [round(statistics.median(ts), 4), round(min(ts), 4), round(max(ts), 4)]


def main():
    reps = 5 if "--profile" in sys.argv else 25
    d = synth3d.make_pair3d(pose=POSE)
    guess = tuple(a + b for a, b in zip(POSE, OFFSET))
    window = search.Window(guess, (3.0, 3.0, math.pi), (0.5, 0.5, 4.0 * math.pi / 180.0))
    out = {}
    with NdtMatcher3D(cell_size=1.0) as t, NdtMatcher3D(cell_size=1.0) as s:
        t.set_target(d["tx"], d["ty"], d["tz"])
        s.set_target(d["sx"], d["sy"], d["sz"])
        out["components"] = int(s.components()[0].size)
        hits = t.search_map(s, *window, k=64)
        out["hits"] = len(hits)
        has_chain = hasattr(t, "align_map_multi")
        for name, knob in (("chain", 1), ("loop", 65)) if has_chain else (("loop", None),):
            if knob is not None:
                t.set_tuning("map_multi_from", knob)
            for k in (8, 64):
                res = t.search_align_map(s, *window, k=k)
                out[f"k{k}_iterations"] = [r.iterations for _, r in res]
                out[f"search_map_k{k}_{name}_ms"] = timed_ms(lambda: t.search_map(s, *window, k=k), reps)
                out[f"search_align_map_k{k}_{name}_ms"] = timed_ms(lambda: t.search_align_map(s, *window, k=k), reps)
            if has_chain:
                for m in (1, 2, 8, 64):
                    poses = [hits[q % len(hits)].pose for q in range(m)]
                    out[f"align_map_multi_m{m}_{name}_ms"] = timed_ms(lambda: t.align_map_multi(s, poses), reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
