"""Timing of ndt2d_align_map_multi and of ndt2d_search_align_map, which refines its hits through it (room50: the 50 m
room of tests/test_gpu_d2d.py, 1065 source components, the loop-closure window of tests/test_gpu_search_map.py).

  search_map / search_align_map, k = 8 and 64   host-timed; their difference is the refinement of the hits
  align_map_multi, m = 1, 2, 8, 64              starts = the poses of the search's hits, once with one chain for all
                                                starts (NDT_TUNE_MAP_MULTI_FROM = 1) and once with one ndt2d_align_map
                                                chain per start (65)

Medians of 25 calls after a warm-up call; one JSON line.  On a library without ndt2d_align_map_multi only the search
figures are printed (the comparison column).  Under `rocprofv3 --kernel-trace --stats` pass --profile (5 calls)."""
import json
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gtsam_ndt_amd import search, synth              # noqa: E402
from gtsam_ndt_amd.matcher import NdtMatcher2D       # noqa: E402

OFFSET = (1.1, -0.9, 0.35)


def med_ms(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    reps = 5 if "--profile" in sys.argv else 25
    d = synth.make_pair(2, n_tgt=20_000, n_src=20_000)
    guess = tuple(a + b for a, b in zip(d["pose"], OFFSET))
    window = search.Window(guess, (2.0, 2.0, math.pi), (0.25, 0.25, 4.0 * math.pi / 180.0))
    out = {}
    with NdtMatcher2D() as t, NdtMatcher2D() as s:
        t.set_target(d["tx"], d["ty"])
        s.set_target(d["sx"], d["sy"])
        out["components"] = int(s.components()[0].size)
        hits = t.search_map(s, *window, k=64)
        out["hits"] = len(hits)
        for k in (8, 64):
            res = t.search_align_map(s, *window, k=k)
            out[f"k{k}_iterations"] = [r.iterations for _, r in res]
            a = med_ms(lambda: t.search_map(s, *window, k=k), reps)
            b = med_ms(lambda: t.search_align_map(s, *window, k=k), reps)
            out[f"search_map_k{k}_ms"], out[f"search_align_map_k{k}_ms"], out[f"refinement_k{k}_ms"] = a, b, b - a
        if hasattr(t, "align_map_multi"):
            for m in (1, 2, 8, 64):
                poses = [hits[q % len(hits)].pose for q in range(m)]
                for name, knob in (("chain", 1), ("loop", 65)):
                    t.set_tuning("map_multi_from", knob)
                    out[f"align_map_multi_m{m}_{name}_ms"] = med_ms(lambda: t.align_map_multi(s, poses), reps)
            t.set_tuning("map_multi_from", 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
