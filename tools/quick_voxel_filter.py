"""The voxel-grid scan filter (ndt2d/ndt3d_voxel_filter_dev) on one device, host call to host result
(the call is synchronous: eight to eleven launches, two read-backs of the header on the way and one at the end), beside
what a caller would write in torch today on the same device arrays in the same run: integer keys from floor(x / leaf),
torch.unique(return_inverse=True), index_add_ of float64 sums and counts, a division, float32 - synchronised at the end.

Shapes: a 64 x 2048 lidar sweep (131 072 points) at leaf 0.2 and 0.5, and the 100 000-point 2D scan of config 2 at leaf
0.1.  Warm-up, then the median (and minimum) of --reps runs.  The kernel split of DESIGN 5.21 is this program under

    rocprofv3 --kernel-trace --stats -d <dir> --output-format csv -- python tools/quick_voxel_filter.py --reps 20 --case K

per shape K.  NDT_HIP_LIB names another build of the library (-DNDT_VOX_MERGE=0: no merging of equal keys within a wave).

    python tools/quick_voxel_filter.py [--reps 30] [--min-points 1] [--case K]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _times_us(fn, reps):
    for _ in range(5):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e6 * float(np.median(t)), 1e6 * float(min(t))


def torch_filter(coords, leaf):
    """The filter as torch operations: float64 sums in the order the atomics happen to take."""
    import torch
    X = torch.stack(coords, dim=1).to(torch.float64)
    idx = torch.floor(X / leaf).to(torch.int64)
    lo = idx.min(dim=0).values
    ext = idx.max(dim=0).values - lo + 1
    key = torch.zeros(X.shape[0], dtype=torch.int64, device=X.device)
    for d in reversed(range(X.shape[1])):
        key = key * ext[d] + (idx[:, d] - lo[d])
    uniq, inverse = torch.unique(key, return_inverse=True)
    sums = torch.zeros((uniq.numel(), X.shape[1]), dtype=torch.float64, device=X.device).index_add_(0, inverse, X)
    cnt = torch.zeros(uniq.numel(), dtype=torch.float64, device=X.device).index_add_(0, inverse, torch.ones_like(X[:, 0]))
    out = (sums / cnt[:, None]).to(torch.float32)
    torch.cuda.synchronize()
    return out


def main():
    import torch
    from gtsam_ndt_amd import synth, synth3d
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--min-points", type=int, default=1)
    ap.add_argument("--case", type=int, default=-1, help="only this shape (0, 1, 2): a kernel trace of its own per shape")
    args = ap.parse_args()
    sweep = synth3d.lidar_scan(101, (0.0,) * 6, 64, 2048).astype(np.float32)
    pair = synth.make_pair(2)
    cases = [("3D 64 x 2048 sweep", NdtMatcher3D, [sweep[:, k] for k in range(3)], 0.2),
             ("3D 64 x 2048 sweep", NdtMatcher3D, [sweep[:, k] for k in range(3)], 0.5),
             ("2D config-2 scan", NdtMatcher2D, [pair["sx"], pair["sy"]], 0.1)]
    if args.case >= 0:
        cases = cases[args.case:args.case + 1]
    print(f"{torch.cuda.get_device_name(0)}; host call to host result, median / minimum of {args.reps} after 5 warm-up calls")
    for name, Matcher, cloud, leaf in cases:
        coords = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.float32)).cuda() for c in cloud]
        n = coords[0].numel()
        torch.cuda.synchronize()
        with Matcher() as m:
            out, info = m.voxel_filter(*coords, leaf, args.min_points, with_info=True)
            ref = torch_filter(coords, leaf)
            if args.min_points == 1:
                assert ref.shape[0] == info.n_out
                diff = float((torch.stack(out, dim=1) - ref).abs().max())       # same order: unique sorts the same keys
            else:
                diff = float("nan")
            again = m.voxel_filter(*coords, leaf, args.min_points)
            same = all(torch.equal(a, b) for a, b in zip(out, again))
            lib = _times_us(lambda: m.voxel_filter(*coords, leaf, args.min_points), args.reps)
            tor = _times_us(lambda: torch_filter(coords, leaf), args.reps)
        print(f"{name}, {n} points, leaf {leaf}: n_out {info.n_out} ({info.n_out / n:.3f} n), invalid {info.n_invalid}; "
              f"library {lib[0]:.1f} / {lib[1]:.1f} us, torch {tor[0]:.1f} / {tor[1]:.1f} us ({tor[0] / lib[0]:.1f}x); "
              f"largest difference to torch's float sums {diff:.2e}; two library calls bit-equal: {same}")


if __name__ == "__main__":
    main()
