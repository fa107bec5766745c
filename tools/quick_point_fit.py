"""Per-point fit and selection (ndt2d_fit_points_dev / ndt2d_select_points_dev) on the config-3 pair:
a 100k-point scan against the 1M-point submap, at the pose the pair was generated with.  Prints the class counts and the
host-to-host time of both calls (synchronous: launches, the table's read-back, the stream wait) next to one evaluate of the
same scan.  The kernel times of DESIGN 5.16 are this program under

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/quick_point_fit.py

k_point_fit, k_point_scan and k_point_select beside k_iterate / k_iterate_first, which the alignments below launch on
the same scan (code this feature does not touch).

    python tools/quick_point_fit.py [--reps 50] [--dim3]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_us(fn, reps):
    for _ in range(5):
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--dim3", action="store_true", help="also the 3D config-5 pair")
    args = ap.parse_args()
    d = synth.make_pair(3)
    cases = [("2D config-3", NdtMatcher2D, ("tx", "ty"), ("sx", "sy"), d, 5.99)]
    if args.dim3:
        cases.append(("3D config-5", NdtMatcher3D, ("tx", "ty", "tz"), ("sx", "sy", "sz"), synth3d.make_pair3d(), 7.81))
    for name, Matcher, tk, sk, pair, max_m in cases:
        tgt = [torch.from_numpy(pair[k]).cuda() for k in tk]
        src = [torch.from_numpy(pair[k]).cuda() for k in sk]
        pose = tuple(pair["pose"])
        torch.cuda.synchronize()
        with Matcher(fixed_iterations=10) as m:
            m.set_target(*tgt)
            fit = m.fit_points(*src, pose, max_m)
            sel, idx, s = m.select_points(*src, pose, max_m)
            print(f"{name}: {src[0].numel()} source points against {tgt[0].numel()} target points, max_m {max_m}: invalid {fit.n_invalid} "
                  f"miss {fit.n_miss} misfit {fit.n_misfit} fit {fit.n_fit} (fitness {fit.fitness:.3f}), fit | miss keeps {s.n_selected}")
            t_fit = _median_us(lambda: m.fit_points(*src, pose, max_m), args.reps)
            t_sel = _median_us(lambda: m.select_points(*src, pose, max_m), args.reps)
            t_eval = _median_us(lambda: m.evaluate(*src, pose), args.reps)
            t_align = _median_us(lambda: m.align(*src, pair["init"]), args.reps)
            print(f"  host to host: fit_points {t_fit:7.1f} us   select_points {t_sel:7.1f} us   evaluate {t_eval:7.1f} us   "
                  f"align, 10 iterations {t_align:7.1f} us   (the Python calls allocate their output tensors)")


if __name__ == "__main__":
    main()
