"""Particle scoring (ndt2d/ndt3d_score_particles*: a team of lanes per pose) against pose-list scoring
(ndt2d/ndt3d_score_poses_dev: one lane per pose) on the same lists, on one device.  The two scenes of
quick_score_poses.py: the 1440-beam scan of quick_search.py's scenario A against the config-3 submap, and
quick_search3d.py's subsampled scan (16384 points) against the config-5 voxel grid.  Particles lie within a metre (and
0.05 rad of roll and pitch, 0.3 rad of heading) of the true pose; m = 256 ... 1048576 of them.
Per list: score_poses, score_particles with teams of 64, of 256 and the default choice, each with the hit counts, and
score_particles(sync=False) followed by one synchronisation.  Times are from host call to host return, the mean, the
least and the largest of --reps calls after a warm-up; the variants alternate inside each repetition so that drift hits
them alike.  The last column is the acceptance condition: the largest score_particles (default) time against the least
score_poses time.
Run under rocprofv3 --kernel-trace --stats for the kernel times (--reps 3 keeps that trace short)."""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gtsam_ndt_amd import synth, synth3d
from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
SIZES = (256, 1024, 2048, 4096, 16384, 65536, 262144, 1048576)


def measure(name, m, scan, truth, spread):
    rng = np.random.default_rng(11)
    n = scan[0].numel()
    print(f"{name}: scan {n} points; host-to-host ms over {reps} repetitions: mean (least .. largest)")

    def team(width, p, **kw):
        m.set_tuning("particle_team", width)
        out = m.score_particles(*scan, p, with_hits=True, **kw)
        m.set_tuning("particle_team", 0)
        return out

    def asynchronous(p):
        out = m.score_particles(*scan, p, with_hits=True, sync=False)
        torch.cuda.synchronize()
        return out

    for k in SIZES:
        p = torch.from_numpy(np.asarray(truth)[None, :] + rng.uniform(-1.0, 1.0, (k, len(truth))) * np.asarray(spread)).cuda()
        torch.cuda.synchronize()
        fns = {"score_poses": lambda: m.score_poses(*scan, p),
               "score_particles, team 64": lambda: team(64, p),
               "score_particles, team 256": lambda: team(256, p),
               "score_particles (default)": lambda: team(0, p),
               "score_particles(sync=False) + sync": lambda: asynchronous(p)}
        lst = m.score_poses(*scan, p)
        got = [fn()[0] for what, fn in fns.items() if what != "score_poses"]
        same = all(torch.equal(g.view(torch.int32), got[0].view(torch.int32)) for g in got)
        rel = float(((got[0].double() - lst.double()).abs() / lst.double().clamp_min(1e-30)).max())
        t = {what: [] for what in fns}
        for _ in range(reps):
            for what, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                t[what].append(1e3 * (time.perf_counter() - t0))
        print(f"  m = {k}: every team width the same bits: {same}; largest relative difference to score_poses {rel:.2e}")
        for what, v in t.items():
            print(f"    {what:38s} {np.mean(v):9.3f}  ({min(v):9.3f} .. {max(v):9.3f})")
        worst, best = max(t["score_particles (default)"]), min(t["score_poses"])
        print(f"    largest score_particles (default) {worst:.3f} ms {'<' if worst < best else '>='} least score_poses {best:.3f} ms")


# ---- 2D: scenario A of quick_search.py
d = synth.make_pair(3)
sc = synth.room_scene(3 + 1000 * (1 * 4 + 2), 50.0, 0.0, -50.0)
P = (d["init"][0] + 0.7, d["init"][1] - 0.4, 0.3)
r, a0, inc = synth.lidar_scan2d(sc, P, n_beams=1440, seed=1)
sx, sy = (torch.from_numpy(a).cuda() for a in synth.scan_points(r, a0, inc))
with NdtMatcher2D() as m:
    m.set_target(torch.from_numpy(d["tx"]).cuda(), torch.from_numpy(d["ty"]).cuda())
    measure("2D, config-3 submap", m, (sx, sy), P, (1.0, 1.0, 0.3))

# ---- 3D: the scan of quick_search3d.py
d = synth3d.make_pair3d()
P = (3.0, -2.5, 0.0, 0.006, -0.005, 1.2)
cloud = synth3d.lidar_scan(102, P).astype(np.float32)
sub = [torch.from_numpy(np.ascontiguousarray(cloud[::8, a])).cuda() for a in range(3)]
with NdtMatcher3D() as m:
    m.set_target(*[torch.from_numpy(d[k]).cuda() for k in ("tx", "ty", "tz")])
    measure("3D, config-5 voxel grid", m, sub, P, (1.0, 1.0, 1.0, 0.05, 0.05, 0.3))
