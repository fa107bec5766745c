"""Map-to-map pose-list scoring (ndt2d/ndt3d_score_map_poses_dev) timings on one device, by HIP events on the target
handle's stream (no profiler attached), warm, the median of --reps calls.
(a) The loop-closure windows of tests/test_gpu_search_map*.py (3D: 90 x 13 x 13, 2D: 90 x 17 x 17) given as lists in flat
    index order, against search_map_scores on the same windows (the lattice kernels, which this list does not touch): the
    same poses and - checked here - the same bits, so the difference is the price of rotating Sigma_i per lane instead
    of once per component and workgroup.
(b) The 1331-pose 3D list over z, roll and pitch of tests/d2d_pose_list_ref.py, against 1331 evaluate_map calls (host
    wall time: each is a synchronous call).
(c) Lists of 256, 4096, 65536 and 2^20 random poses within a metre (3D: 0.5 m in z, 0.1 rad of roll and pitch) and any
    heading of the generating pose.
NDT_HIP_LIB names another build of the library (gtsam_ndt_amd/_lib.py), such as one with another kMapPoses3InFlight."""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

import d2d_pose_list_ref as P
from gtsam_ndt_amd import search
from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
DEG = math.pi / 180.0


def timed(t, fn):
    """median and minimum GPU-side milliseconds of fn() on t's stream, after three warm-up calls"""
    st = torch.cuda.ExternalStream(t.stream)
    out = []
    for _ in range(reps + 3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        fn()
        e1.record(st)
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out[3:])), float(min(out[3:]))


def dev(poses):
    return torch.from_numpy(np.ascontiguousarray(poses, dtype=np.float64)).cuda()


def measure(name, t, s, window, centre, spread):
    n_comp = s.components()[0].size
    lat = dev(P.lattice_list(window))
    vol = t.search_map_scores(s, *window)
    same = torch.equal(vol.reshape(-1).view(torch.int32), t.score_map_poses(s, lat).view(torch.int32))
    print(f"{name}: {n_comp} source components, window {tuple(vol.shape)} = {vol.numel()} poses; "
          f"list in lattice order == volume bit for bit: {same}")
    rows = [("search_map_scores (lattice kernel)", vol.numel(), timed(t, lambda: t.search_map_scores(s, *window))),
            ("score_map_poses, the lattice as a list", vol.numel(), timed(t, lambda: t.score_map_poses(s, lat))),
            ("score_map_poses with counts, the same list", vol.numel(), timed(t, lambda: t.score_map_poses(s, lat, with_hits=True)))]
    rng = np.random.default_rng(11)
    for m in (256, 4096, 65536, 1 << 20):       # (2^20: several waves per SIMD, where the kernels' occupancy shows)
        lst = dev(np.asarray(centre)[None, :] + rng.uniform(-1.0, 1.0, (m, len(centre))) * np.asarray(spread))
        rows.append((f"score_map_poses, {m} random poses", m, timed(t, lambda lst=lst: t.score_map_poses(s, lst))))
    for what, m, (med, best) in rows:
        print(f"  {what:46s} median {med:8.3f} ms  min {best:8.3f} ms   {n_comp * m / med / 1e6:7.2f} G component-pose terms/s")


# ---- 3D: the small pair at 1 m, the loop window of tests/test_gpu_search_map3d.py
d = P.pair3("small")
guess = tuple(a + b for a, b in zip(P.POSE3, (1.6, -1.3, 0.0, 0.0, 0.0, 0.5)))
with NdtMatcher3D() as t, NdtMatcher3D() as s:
    t.set_target(d["tx"], d["ty"], d["tz"])
    s.set_target(d["sx"], d["sy"], d["sz"])
    measure("3D, small pair at 1 m", t, s, search.Window(guess, (3.0, 3.0, math.pi), (0.5, 0.5, 4.0 * DEG)), P.POSE3,
            (1.0, 1.0, 0.5, 0.1, 0.1, math.pi))

# ---- 3D: the list over z, roll and pitch against one evaluate_map call per pose
d = P.pair3("small", P.LOOP_POSE3)
poses = P.loop_list3()
with NdtMatcher3D() as t, NdtMatcher3D() as s:
    t.set_target(d["tx"], d["ty"], d["tz"])
    s.set_target(d["sx"], d["sy"], d["sz"])
    lst = dev(poses)
    med, best = timed(t, lambda: t.score_map_poses(s, lst))
    t0 = time.perf_counter()
    t.score_map_poses(s, lst)
    wall = time.perf_counter() - t0
    rows = [tuple(float(v) for v in p) for p in poses]
    t.evaluate_map(s, rows[0])
    t0 = time.perf_counter()
    ev = [t.evaluate_map(s, p)[2] for p in rows]
    loop = time.perf_counter() - t0
    got = t.score_map_poses(s, lst).cpu().numpy()
    rel = float(np.max(np.abs(got - np.array(ev)) / np.maximum(np.abs(ev), 1e-30)))
    print(f"3D, {len(rows)} poses over z, roll and pitch: score_map_poses {med:.3f} ms on the stream (min {best:.3f}), "
          f"{1e3 * wall:.3f} ms host call to return; {len(rows)} evaluate_map calls {1e3 * loop:.1f} ms; "
          f"largest relative difference {rel:.1e}")

# ---- 2D: the 50 m room at 0.5 m, the loop window of tests/test_gpu_search_map.py
d = P.pair2("room50")
guess = tuple(a + b for a, b in zip(d["pose"], (1.1, -0.9, 0.35)))
with NdtMatcher2D() as t, NdtMatcher2D() as s:
    t.set_target(d["tx"], d["ty"])
    s.set_target(d["sx"], d["sy"])
    measure("2D, 50 m room at 0.5 m", t, s, search.Window(guess, (2.0, 2.0, math.pi), (0.25, 0.25, 4.0 * DEG)), d["pose"],
            (1.0, 1.0, math.pi))
