"""Sweep de-skewing timings on one device by HIP events on torch's current stream (no profiler attached), warm: the three
kernels (k_polar_to_points_deskew at 1440 and 7200 beams, k_range_image_to_points_deskew at 64 x 2048,
k_deskew_points<2> / <3> on the same point counts) beside the plain conversions on the same shapes in the same process.
Two figures per call: the events around ONE call (median and minimum of --reps; this includes the launch), and the
events around 50 calls issued back to back, divided by 50 (what a stream that is kept busy pays per call; when the
host issues slower than the device runs, this is the host's issue rate).  DESIGN.md section 5.20."""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from gtsam_ndt_amd.matcher import deskew_points, polar_to_points, range_image_to_points

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
BURST = 50
MOTION2, MOTION3 = (0.25, 0.05, 0.08), (0.5, 0.1, 0.02, 0.01, -0.01, 0.12)


def timed(fn):
    one, burst = [], []
    for k in range(reps + 3):
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        fn()
        e1.record()
        for _ in range(BURST):
            fn()
        e2.record()
        e2.synchronize()
        if k >= 3:
            one.append(e0.elapsed_time(e1) * 1e3)
            burst.append(e1.elapsed_time(e2) * 1e3 / BURST)
    return float(np.median(one)), float(min(one)), float(np.median(burst))


def report(rows):
    for what, n, (med, best, burst) in rows:
        print(f"  {what:44s} {n:7d} points: one call median {med:7.1f} us  min {best:7.1f} us   back to back {burst:6.1f} us / call")


rng = np.random.default_rng(3)
rows = []
for n in (1440, 7200):
    r = torch.from_numpy(rng.uniform(0.5, 30.0, n).astype(np.float32)).cuda()
    f = torch.from_numpy(rng.uniform(0.0, 1.0, n).astype(np.float32)).cuda()
    inc = 2.0 * math.pi / n
    x, y = polar_to_points(r, -math.pi, inc, 0.05, 30.0)
    rows.append(("polar_to_points (plain)", n, timed(lambda: polar_to_points(r, -math.pi, inc, 0.05, 30.0))))
    rows.append(("polar_to_points, motion", n, timed(lambda: polar_to_points(r, -math.pi, inc, 0.05, 30.0, motion=MOTION2))))
    rows.append(("deskew_points 2D, in place", n, timed(lambda: deskew_points((x, y), f, MOTION2, 1.0, out=(x, y)))))
ne, na = 64, 2048
n = ne * na
r = torch.from_numpy(rng.uniform(0.5, 100.0, (ne, na)).astype(np.float32)).cuda()
f = torch.from_numpy(rng.uniform(0.0, 1.0, n).astype(np.float32)).cuda()
el = np.deg2rad(np.linspace(-24.0, 20.0, ne))
inc = 2.0 * math.pi / na
p = range_image_to_points(r, el, 0.5 * inc, inc, 0.05, 100.0)
rows.append(("range_image_to_points 64 x 2048 (plain)", n, timed(lambda: range_image_to_points(r, el, 0.5 * inc, inc, 0.05, 100.0))))
rows.append(("range_image_to_points 64 x 2048, motion", n,
             timed(lambda: range_image_to_points(r, el, 0.5 * inc, inc, 0.05, 100.0, motion=MOTION3))))
rows.append(("deskew_points 3D, in place", n, timed(lambda: deskew_points(p, f, MOTION3, 1.0, out=p))))
print(f"HIP events on torch's current stream, {reps} repetitions after 3 warm-up rounds, bursts of {BURST}")
report(rows)
