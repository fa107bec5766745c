"""The 3D neighbourhood option (ndt3d_set_neighbourhood): what 7 costs and what it is worth.

cost   fixed-30 iterations/s of the config-5 pair (131072 points) on one launch chain (40 back-to-back asynchronous
       alignments between two events on the handle's stream) and of 64 scans per chain (align_multi_scan, host clock
       around the synchronous call), with neighbourhood 1 and 7 on ONE handle, alternating, `--reps` rounds each: median
       and min .. max.  On a library without the option (the parent commit) only 1 is measured, by the same code.
worth  16 seeded starts spread up to 1.5 voxels / 0.15 rad from the generating pose of make_pair3d(32, 512): how many
       a converged-mode alignment brings back to it (5e-3 m, 1e-3 rad) and the mean iteration count, with 1 and 7, on
       the device and (--cpu: no device needed) on the float64 restatement tests/ndt3d_nb_ref.py.

    python tools/quick_nb3d.py [cost | worth | all] [--reps 7] [--cpu]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 30


def _summary(v):
    return f"median {np.median(v):9.0f}  min {min(v):9.0f}  max {max(v):9.0f}"


def cost(reps):
    import torch
    from gtsam_ndt_amd import synth3d
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    has = hasattr(NdtMatcher3D, "set_neighbourhood")
    nbs = (1, 7) if has else (1,)
    print(f"library {os.environ.get('NDT_HIP_LIB', 'of this tree')}; neighbourhood option {'present' if has else 'absent'}")
    d = synth3d.make_pair3d()
    s = [torch.from_numpy(d[k]).cuda() for k in ("sx", "sy", "sz")]
    for mode in (0, 1):
        with NdtMatcher3D(fixed_iterations=K, hessian_mode=mode) as m:
            m.set_target(d["tx"], d["ty"], d["tz"])
            st = torch.cuda.ExternalStream(m.stream)

            def chain(calls):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for _ in range(calls):
                    m.align_async(*s, d["init"], producer_complete=True)
                e1.record(st)
                e1.synchronize()
                m.finish()
                return calls * K / (1e-3 * e0.elapsed_time(e1))

            def multi(calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(calls):
                    m.align_multi_scan([tuple(s)] * 64, [d["init"]] * 64)
                return calls * 64 * K / (time.perf_counter() - t0)

            for name, fn, calls in (("one chain", chain, 40), ("64 scans per chain", multi, 5)):
                rate = {nb: [] for nb in nbs}
                for nb in nbs:                                         # every shape and graph once before the clock
                    if has:
                        m.set_neighbourhood(nb)
                    fn(3)
                for _ in range(reps):
                    for nb in nbs:
                        if has:
                            m.set_neighbourhood(nb)
                        rate[nb].append(fn(calls))
                for nb in nbs:
                    print(f"mode {mode}  {name:18s}  neighbourhood {nb}: iterations/s {_summary(rate[nb])}")
                if has:
                    print(f"mode {mode}  {name:18s}  time of 7 / time of 1 = {np.median(rate[1]) / np.median(rate[7]):.2f}")


def worth(cpu):
    from gtsam_ndt_amd import synth3d
    d = synth3d.make_pair3d(n_elev=32, n_azim=512)
    S = (d["sx"], d["sy"], d["sz"])
    rng = np.random.default_rng(2024)
    starts = []
    for _ in range(16):
        u, w = rng.normal(size=3), rng.normal(size=3)
        off = np.concatenate([u / np.linalg.norm(u) * rng.uniform(0, 1.5 * d["cell"]), w / np.linalg.norm(w) * rng.uniform(0, 0.15)])
        starts.append(tuple(np.array(d["pose"]) + off))

    def report(where, nb, results):
        ok = [np.abs(np.array(p[:3]) - d["pose"][:3]).max() < 5e-3 and np.abs(np.array(p[3:]) - d["pose"][3:]).max() < 1e-3
              for p, _ in results]
        print(f"{where:12s} neighbourhood {nb}: {sum(ok):2d} of 16 recovered; mean iterations {np.mean([it for _, it in results]):5.1f} "
              f"(recovered ones {np.mean([it for (_, it), k in zip(results, ok) if k]) if any(ok) else float('nan'):5.1f})")

    if cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import ndt3d_nb_ref as N
        from oracle import ndt3d as o
        prm = o.Ndt3Params()
        g = o.build_grid3(d["tx"], d["ty"], d["tz"], prm)
        for nb in (1, 7):
            rs = [N.align3_nb(g, *S, p, prm, nb) for p in starts]
            report("restatement", nb, [(r["pose"], r["iterations"]) for r in rs])
        return
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    with NdtMatcher3D() as m:
        m.set_target(d["tx"], d["ty"], d["tz"])
        for nb in (1, 7):
            m.set_neighbourhood(nb)
            rs = [m.align(*S, p) for p in starts]
            report("device", nb, [(r.pose, r.iterations) for r in rs])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all", choices=("cost", "worth", "all"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--cpu", action="store_true", help="worth: the float64 restatement instead of the device")
    a = ap.parse_args()
    if a.what in ("cost", "all") and not a.cpu:
        cost(a.reps)
    if a.what in ("worth", "all"):
        worth(a.cpu)


if __name__ == "__main__":
    main()
