"""Exhaustive 3D pose search (ndt3d_search_dev) timings on one device: a 64-beam lidar scan taken 3.9 m and 69 degrees
from the map origin, every 8th point of it (16384 points), against the config-5 voxel grid; window +-3 m x +-3 m x full
turn at 0.25 m / 1 deg (25 x 25 x 360 = 225000 poses), z / roll / pitch pinned to 0.  Prints the time from host call to
host result of search_scores(), search() and search_align() (k = 8) with the subsampled scan, of search() followed by
align_multi_start() on the full scan (the relocaliser), and point-pose evaluations per second.
Run under rocprofv3 --kernel-trace --stats for the kernel times (--reps 3 keeps that trace short)."""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gtsam_ndt_amd import synth3d
from gtsam_ndt_amd.matcher import NdtMatcher3D

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
DEG = math.pi / 180.0

d = synth3d.make_pair3d()
P = (3.0, -2.5, 0.0, 0.006, -0.005, 1.2)
scan = synth3d.lidar_scan(102, P).astype(np.float32)
full = [torch.from_numpy(np.ascontiguousarray(scan[:, a])).cuda() for a in range(3)]
sub = [torch.from_numpy(np.ascontiguousarray(scan[::8, a])).cuda() for a in range(3)]
guess = (P[0] + 1.5, P[1] - 1.25, 0.0, 0.0, 0.0, P[5] + 0.8)
win = (guess, (3.0, 3.0, math.pi), (0.25, 0.25, DEG))


def relocalise(m):
    hits = m.search(*sub, *win, k=8)
    return hits, m.align_multi_start(*full, [h.pose for h in hits])


with NdtMatcher3D() as m:
    info = m.set_target(*[torch.from_numpy(d[k]).cuda() for k in ("tx", "ty", "tz")])
    torch.cuda.synchronize()
    vol = m.search_scores(*sub, *win)
    poses = vol.numel()
    t = {}
    for what, fn in (("scores", lambda: m.search_scores(*sub, *win)), ("search", lambda: m.search(*sub, *win, k=8)),
                     ("search_align", lambda: m.search_align(*sub, *win, k=8)), ("relocalise", lambda: relocalise(m))):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        t[what] = (time.perf_counter() - t0) / reps
    hits, refined = relocalise(m)
    best = max((r for r in refined if r.status == 0), key=lambda r: r.score, default=None)
n = sub[0].numel()
print(f"config-5 grid {info.width} x {info.height} x {info.depth}, {info.n_valid} valid voxels; scan {full[0].numel()} points, "
      f"searched with {n}; {tuple(vol.shape)} = {poses} poses")
print(f"  search_scores {1e3 * t['scores']:.3f} ms | search {1e3 * t['search']:.3f} ms | search_align {1e3 * t['search_align']:.3f} ms"
      f" | search + align_multi_start(full scan) {1e3 * t['relocalise']:.3f} ms  (host call to host result, mean of {reps})")
print(f"  {n * poses / t['scores'] / 1e9:.1f} G point-pose evaluations/s")
print(f"  best hit {hits[0]}")
print(f"  best refined {best.pose if best else None} (truth {P})")
