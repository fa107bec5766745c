"""Submap merging (ndt2d_merge_map / ndt3d_merge_map): host-to-host time of merge_map / unmerge_map of
the config-3 submap (2D, 1M points, 0.5 m cells) and the config-5 voxel grid (3D, 1 m voxels) into a reserved grid of the
same cell size at a general pose, next to what a caller with the raw points does - add_target_points / remove_target_points
of the same device-resident points with the same pose (code this feature does not touch: the parent commit's numbers) - and
the bytes-read floor of the merge kernel (src's sums once, at the 6.3 TB/s a streaming copy reaches on one MI355X).  All
calls are synchronous; the times include the finalise of the destination and its host round trip.  Merge and unmerge
alternate, so the destination never fills up.

    python tools/quick_merge.py [--reps 20]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_BPS = 6.3e12


def _median_pair_us(do, undo, reps):
    """Median times of do() and undo(), called in turn."""
    for _ in range(3):
        do()
        undo()
    t = [[], []]
    for _ in range(reps):
        for k, fn in enumerate((do, undo)):
            t0 = time.perf_counter()
            fn()
            t[k].append(time.perf_counter() - t0)
    return 1e6 * float(np.median(t[0])), 1e6 * float(np.median(t[1]))


def main():
    import torch
    from gtsam_ndt_amd import synth, synth3d
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    reps = ap.parse_args().reps
    d = synth.make_pair(3)
    d3 = synth3d.make_pair3d()
    cases = (("2D config-3 submap", NdtMatcher2D, 0.5, 48, [d[k] for k in ("tx", "ty")], (0.37, -0.21, 0.03)),
             ("3D config-5 grid", NdtMatcher3D, 1.0, 80, [d3[k] for k in ("tx", "ty", "tz")], (0.37, -0.21, 0.12, 0.01, -0.02, 0.03)))
    for name, Matcher, c, cell_bytes, host, pose in cases:
        pts = [torch.from_numpy(a).cuda() for a in host]
        lo = [float(a.min()) - 8.0 for a in host]
        hi = [float(a.max()) + 8.0 for a in host]
        with Matcher(cell_size=c) as src, Matcher(cell_size=c) as merged, Matcher(cell_size=c) as added:
            src.set_target(*pts)
            for m in (merged, added):
                if len(host) == 2:
                    m.reserve_target(lo[0], lo[1], hi[0], hi[1])
                else:
                    m.reserve_target(lo, hi)
            info = src.grid_info()
            ncell = info.width * info.height * getattr(info, "depth", 1)
            filled = int(np.count_nonzero(src.grid()[0]))
            read = ncell * cell_bytes
            print(f"{name}: {pts[0].numel()} points, {ncell} cells of {c} m ({filled} hold points), {read / 1e6:.1f} MB of sums "
                  f"(read once: {1e6 * read / HBM_BPS:.1f} us at {HBM_BPS / 1e12:.1f} TB/s)")
            outside = merged.merge_map(src, pose)
            merged.unmerge_map(src, pose)
            t_merge, t_unmerge = _median_pair_us(lambda: merged.merge_map(src, pose), lambda: merged.unmerge_map(src, pose), reps)
            t_add, t_remove = _median_pair_us(lambda: added.add_target_points(*pts, pose=pose),
                                              lambda: added.remove_target_points(*pts, pose=pose), reps)
            print(f"  merge_map {t_merge:8.1f} us   unmerge_map {t_unmerge:8.1f} us   ({outside} points outside)")
            print(f"  add_target_points of the points {t_add:8.1f} us   remove_target_points {t_remove:8.1f} us")


if __name__ == "__main__":
    main()
