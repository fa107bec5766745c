"""Scratch: aggregate fixed-30 iteration rate of N handles on the config 3 pair, each with its own grid.
default        N = 1, 2, 4, 8 handles driven from N host threads, 200 alignments each
--round-robin  N = 1, 2, 3 handles driven round-robin from ONE host thread, as a handle with more launch chains would
               be: with the default two chains per handle that is 2, 4 and 6 chains.  7 samples of 100 alignments in all
               (the counts alternating inside every sample), median (min - max) of the aggregate time per launch, and
               the host's share: the time the enqueueing loop alone took, per alignment.
--chains C     set NDT_TUNE_ASYNC_CHAINS = C on every handle (a library that has the knob)
NDT_HIP_LIB selects the library."""
import os, sys, threading, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gtsam_ndt_amd import synth
from gtsam_ndt_amd.matcher import NdtMatcher2D

CHAINS = int(sys.argv[sys.argv.index("--chains") + 1]) if "--chains" in sys.argv else None
d = synth.make_pair(3)
tx, ty, sx, sy = (torch.from_numpy(d[k]).cuda() for k in ("tx", "ty", "sx", "sy"))
torch.cuda.synchronize()
K, STEPS = 30, 200


def handles(n):
    ms = [NdtMatcher2D(fixed_iterations=K) for _ in range(n)]
    for m in ms:
        m.set_target(tx, ty)
        if CHAINS is not None:
            m.set_tuning("async_chains", CHAINS)
        m.align_async(sx, sy, d["init"]); m.finish()
    return ms


def threaded():
    for n in (1, 2, 4, 8):
        ms = handles(n)
        go = threading.Barrier(n + 1)
        def work(m):
            go.wait()
            for _ in range(STEPS):
                m.align_async(sx, sy, d["init"])
            m.finish()
        th = [threading.Thread(target=work, args=(m,)) for m in ms]
        for t in th: t.start()
        go.wait(); t0 = time.perf_counter()
        for t in th: t.join()
        el = time.perf_counter() - t0
        print(f"{n} handles: {n * STEPS * K / el:,.0f} iterations/s aggregate ({1e6 * el / (STEPS * (K + 1)):.2f} us per launch per handle)")
        for m in ms: m.close()


def round_robin():
    REPEATS, CALLS, COUNTS = 7, 100, (1, 2, 3)
    ms = handles(max(COUNTS))
    us = {n: [] for n in COUNTS}
    host = {n: [] for n in COUNTS}
    for rep in range(REPEATS + 1):              # sample 0 is the warm-up
        for n in COUNTS:
            t0 = time.perf_counter()
            for c in range(CALLS):
                ms[c % n].align_async(sx, sy, d["init"], producer_complete=True)
            t1 = time.perf_counter()
            for m in ms[:n]: m.finish()
            el = time.perf_counter() - t0
            if rep:
                us[n].append(1e6 * el / (CALLS * (K + 1)))
                host[n].append(1e6 * (t1 - t0) / CALLS)
    per = "default" if CHAINS is None else str(CHAINS)
    for n in COUNTS:
        a, h = np.array(us[n]), np.array(host[n])
        print(f"{n} handles ({per} chains each), one thread: {np.median(a):.3f} us per launch in aggregate (min {a.min():.3f}, "
              f"max {a.max():.3f}; {REPEATS} samples of {CALLS} alignments) = {np.median(a) * (K + 1):.1f} us per alignment = "
              f"{K / (K + 1) / np.median(a) * 1e3:.1f}k iterations/s; host enqueue {np.median(h):.1f} us per alignment; "
              f"{os.environ.get('NDT_HIP_LIB', 'product library')}")
    for m in ms: m.close()


if "--round-robin" in sys.argv:
    round_robin()
else:
    threaded()
