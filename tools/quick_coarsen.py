"""Submap coarsening (ndt2d_coarsen_map / ndt3d_coarsen_map): host-to-host time of coarsen_into for the
config-3 submap (2D, 1M points, 0.5 m cells -> 1 m and 2 m) and the config-5 voxel grid (3D, 1 m -> 2 m and 4 m), next to
what a caller does today - a set_target at the coarse cell from the device-resident points - and the bytes-read roofline
of the coarsen kernel (src's sums once, at the 6.3 TB/s a streaming copy reaches on one MI355X).  Both calls are
synchronous; the times include the finalise of the coarse grid and its host round trip.

    python tools/quick_coarsen.py [--reps 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BPS = 6.3e12


def _median_us(fn, reps):
    for _ in range(3):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(t))


def main():
    import torch
    from gtsam_ndt_amd import synth, synth3d
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    reps = ap.parse_args().reps
    d = synth.make_pair(3)
    d3 = synth3d.make_pair3d()
    cases = (("2D config-3 submap", NdtMatcher2D, 0.5, 48, [torch.from_numpy(d[k]).cuda() for k in ("tx", "ty")]),
             ("3D config-5 grid", NdtMatcher3D, 1.0, 80, [torch.from_numpy(d3[k]).cuda() for k in ("tx", "ty", "tz")]))
    for name, Matcher, c, cell_bytes, pts in cases:
        with Matcher(cell_size=c) as src:
            src.set_target(*pts)
            info = src.grid_info()
            ncell = info.width * info.height * getattr(info, "depth", 1)
            read = ncell * cell_bytes
            print(f"{name}: {pts[0].numel()} points, {ncell} cells of {c} m, {read / 1e6:.1f} MB of sums "
                  f"(read once: {1e6 * read / HBM_BPS:.1f} us at {HBM_BPS / 1e12:.1f} TB/s)")
            for f in (2, 4):
                with Matcher(cell_size=f * c, eig_ratio=0.03) as dst, Matcher(cell_size=f * c, eig_ratio=0.03) as rebuilt:
                    t_coarsen = _median_us(lambda: src.coarsen_into(dst), reps)
                    t_rebuild = _median_us(lambda: rebuilt.set_target(*pts), reps)
                    print(f"  f = {f}: coarsen_into {t_coarsen:8.1f} us   set_target at {f * c} m from the points {t_rebuild:8.1f} us   "
                          f"valid cells {dst.grid_info().n_valid} / {rebuilt.grid_info().n_valid}")


if __name__ == "__main__":
    main()
