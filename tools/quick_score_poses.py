"""Pose-list scoring (ndt2d/ndt3d_score_poses_dev) timings on one device, against the lattice kernel of the exhaustive
search on the same poses.  2D: the 1440-beam scan of quick_search.py's scenario A against the config-3 submap, window
+-3 m x +-3 m x full turn at 0.1 m / 1 deg (1.34M poses).  3D: quick_search3d.py's subsampled scan (16384 points) against
the config-5 voxel grid, +-3 m x +-3 m x full turn at 0.25 m / 1 deg (225000 poses), z / roll / pitch pinned.
Per dimension: search_scores() on the window, then score_poses() on the window's poses as a list in three orders - the
lattice's flat order (checked bit for bit against the volume), shuffled, and sorted by (x, y) - and on 4096 and 65536
random particles within a metre (and 0.05 rad of roll and pitch, 0.3 rad of heading) of the true pose.  Times are from
host call to host return (every call returns once its output is complete), the mean of --reps calls after a warm-up; the
variants alternate inside each repetition so that drift hits them alike.
Run under rocprofv3 --kernel-trace --stats for the kernel times (--reps 3 keeps that trace short)."""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gtsam_ndt_amd import search, synth, synth3d
from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
DEG = math.pi / 180.0


def lattice_list(window):
    c = window[0]
    xs, ys, th = search.lattice(window)
    T, Y, X = np.meshgrid(th, ys, xs, indexing="ij")
    cols = [X.ravel(), Y.ravel()] + ([np.full(X.size, c[a]) for a in (2, 3, 4)] if len(c) == 6 else []) + [T.ravel()]
    return np.stack(cols, axis=1)


def measure(name, m, scan, window, truth, spread):
    rng = np.random.default_rng(11)
    poses = lattice_list(window)
    orders = {"lattice order": poses, "shuffled": poses[rng.permutation(len(poses))],
              "sorted by (x, y)": poses[np.lexsort((poses[:, 1], poses[:, 0]))]}
    for k in (4096, 65536):
        orders[f"{k} particles"] = np.asarray(truth)[None, :] + rng.uniform(-1.0, 1.0, (k, len(truth))) * np.asarray(spread)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in orders.items()}
    torch.cuda.synchronize()
    fns = {"search_scores (lattice kernel)": lambda: m.search_scores(*scan, *window)}
    fns.update({f"score_poses, {k}": (lambda p=p: m.score_poses(*scan, p)) for k, p in dev.items()})
    vol = m.search_scores(*scan, *window)
    same = torch.equal(vol.reshape(-1).view(torch.int32), m.score_poses(*scan, dev["lattice order"]).view(torch.int32))
    for fn in fns.values():
        fn()
    t = dict.fromkeys(fns, 0.0)
    for _ in range(reps):
        for what, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            t[what] += time.perf_counter() - t0
    n = scan[0].numel()
    print(f"{name}: scan {n} points, window {tuple(vol.shape)} = {vol.numel()} poses; list in lattice order == volume bit for bit: {same}")
    for what, s in t.items():
        count = vol.numel() if "particles" not in what else int(what.split()[1])
        print(f"  {what:42s} {1e3 * s / reps:9.3f} ms   {n * count / (s / reps) / 1e9:7.1f} G point-pose evaluations/s")


# ---- 2D: scenario A of quick_search.py
d = synth.make_pair(3)
sc = synth.room_scene(3 + 1000 * (1 * 4 + 2), 50.0, 0.0, -50.0)
P = (d["init"][0] + 0.7, d["init"][1] - 0.4, 0.3)
r, a0, inc = synth.lidar_scan2d(sc, P, n_beams=1440, seed=1)
sx, sy = (torch.from_numpy(a).cuda() for a in synth.scan_points(r, a0, inc))
with NdtMatcher2D() as m:
    m.set_target(torch.from_numpy(d["tx"]).cuda(), torch.from_numpy(d["ty"]).cuda())
    measure("2D, config-3 submap", m, (sx, sy), (d["init"], (3.0, 3.0, math.pi), (0.1, 0.1, DEG)), P, (1.0, 1.0, 0.3))

# ---- 3D: the scan and window of quick_search3d.py
d = synth3d.make_pair3d()
P = (3.0, -2.5, 0.0, 0.006, -0.005, 1.2)
cloud = synth3d.lidar_scan(102, P).astype(np.float32)
sub = [torch.from_numpy(np.ascontiguousarray(cloud[::8, a])).cuda() for a in range(3)]
guess = (P[0] + 1.5, P[1] - 1.25, 0.0, 0.0, 0.0, P[5] + 0.8)
with NdtMatcher3D() as m:
    m.set_target(*[torch.from_numpy(d[k]).cuda() for k in ("tx", "ty", "tz")])
    measure("3D, config-5 voxel grid", m, sub, (guess, (3.0, 3.0, math.pi), (0.25, 0.25, DEG)), P,
            (1.0, 1.0, 1.0, 0.05, 0.05, 0.3))
