"""Exhaustive pose search (ndt2d_search_dev) timings on one device: scenario A = a 1440-beam lidar scan against the
config-3 1M-point submap, scenario B = the same kind of scan against a config-2 100k-point target; window +-3 m x +-3 m
x full turn at 0.1 m / 1 deg (61 x 61 x 360 = 1.34M poses).  Prints, per scenario, the time from host call to host
hits of search() and search_align() (k = 8), the time of search_scores() alone, and point-pose evaluations per second.
Run under rocprofv3 --kernel-trace --stats for the kernel times (--reps 3 keeps that trace short)."""
import math
import sys
import time

sys.path.insert(0, ".")
import numpy as np
import torch

from gtsam_ndt_amd import synth
from gtsam_ndt_amd.matcher import NdtMatcher2D

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
DEG = math.pi / 180.0


def scenario(cfg):
    d = synth.make_pair(cfg)
    L = 50.0
    if cfg == 3:       # the source room of config 3: room (2, 1) of the 4 x 4 submap
        half = 2 * L
        sc = synth.room_scene(3 + 1000 * (1 * 4 + 2), L, 2 * L - half, 1 * L - half)
    else:
        sc = synth.room_scene(2, L, -0.5 * L, -0.5 * L)
    P = (d["init"][0] + 0.7, d["init"][1] - 0.4, 0.3)
    r, a0, inc = synth.lidar_scan2d(sc, P, n_beams=1440, seed=1)
    sx, sy = synth.scan_points(r, a0, inc)
    return d, sx, sy, P


for cfg, name in ((3, "A"), (2, "B")):
    d, sx_h, sy_h, P = scenario(cfg)
    n_valid = int(np.isfinite(sx_h).sum())
    sx, sy = torch.from_numpy(sx_h).cuda(), torch.from_numpy(sy_h).cuda()
    win = (d["init"], (3.0, 3.0, math.pi), (0.1, 0.1, DEG))
    with NdtMatcher2D() as m:
        m.set_target(torch.from_numpy(d["tx"]).cuda(), torch.from_numpy(d["ty"]).cuda())
        torch.cuda.synchronize()
        vol = m.search_scores(sx, sy, *win)
        poses = vol.numel()
        hits = m.search(sx, sy, *win, k=8)
        t = {}
        for what, fn in (("scores", lambda: m.search_scores(sx, sy, *win)), ("search", lambda: m.search(sx, sy, *win, k=8)),
                         ("search_align", lambda: m.search_align(sx, sy, *win, k=8))):
            fn()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            t[what] = (time.perf_counter() - t0) / reps
        best = max(m.search_align(sx, sy, *win, k=8), key=lambda hr: hr[1].score if hr[1].converged else -1.0)
    ev = sx.numel() * poses
    print(f"scenario {name} (config {cfg}, {d['tx'].size} target points): scan {sx.numel()} beams / {n_valid} valid, "
          f"{tuple(vol.shape)} = {poses} poses")
    print(f"  search_scores {1e3 * t['scores']:.3f} ms | search {1e3 * t['search']:.3f} ms | "
          f"search_align {1e3 * t['search_align']:.3f} ms  (host call to host result, mean of {reps})")
    print(f"  {ev / t['scores'] / 1e9:.1f} G point-pose evaluations/s over the whole scan "
          f"({n_valid * poses / t['scores'] / 1e9:.1f} G/s over its valid points)")
    print(f"  best hit {hits[0]}; best aligned {best[1].pose} (truth {P}), status {best[1].status}")
