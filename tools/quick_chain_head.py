"""The time per k_iterate launch of a chain on the headline pair (config 3: 1M-point target, 100k-point scan, 30 fixed
iterations = 31 launches per alignment), with one launch chain (NDT_TUNE_ASYNC_LANES = 1: what a change to the head of
the kernel moves) and with two (the throughput bench.py's headline reports).  100 back-to-back asynchronous alignments
per sample, REPEATS samples each, lanes alternating so that drift hits both alike.  Host clock around the 100 calls and
the finish, divided by the launches: the figure is launch + boundary and carries the host's share of enqueueing 100
k_begin + graph launches (the device is the slower side here, so it is small, but it is in there) - a chain's time per
launch, good for comparing two builds, not the bare latency of a launch.
NDT_HIP_LIB selects the library, to compare two builds in one session.
--fused 0 | 1: set NDT_TUNE_FUSED_BEGIN (a library that has the knob): 0 = k_begin + K + 1 launches, 1 = the first launch
carries the call's arguments (K + 1 kernels in all).  Either way the time is divided by K + 1 launches, so that the
figures of the two protocols compare as time per alignment / (K + 1); the time per alignment is printed as well.
--lane-fork 0 | 1: set NDT_TUNE_LANE_FORK (a library that has the knob): 0 = lane 1 forks from the handle's stream only
behind non-chain work, 1 = at every pair.  It moves the two-lane figure; the one-lane figure must not move.
--chains N[,N...]: the counts to time, set with NDT_TUNE_ASYNC_CHAINS (a library that has the knob; 1..4), alternating
inside every sample like the two lanes of the default run (which sets NDT_TUNE_ASYNC_LANES = 1, 2 and so runs on every
library).  The host's share is printed too: the time the loop of 100 enqueueing calls alone took, per alignment."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from gtsam_ndt_amd import synth
from gtsam_ndt_amd.matcher import NdtMatcher2D
REPEATS, CALLS, K = 7, 100, 30
FUSED = int(sys.argv[sys.argv.index("--fused") + 1]) if "--fused" in sys.argv else None
LANE_FORK = int(sys.argv[sys.argv.index("--lane-fork") + 1]) if "--lane-fork" in sys.argv else None
CHAINS = [int(c) for c in sys.argv[sys.argv.index("--chains") + 1].split(",")] if "--chains" in sys.argv else None
KNOB, COUNTS = ("async_chains", CHAINS) if CHAINS else ("async_lanes", [1, 2])
d = synth.make_pair(3)
tx, ty = torch.from_numpy(d["tx"]).cuda(), torch.from_numpy(d["ty"]).cuda()
sx, sy = torch.from_numpy(d["sx"]).cuda(), torch.from_numpy(d["sy"]).cuda()
torch.cuda.synchronize()
us = {c: [] for c in COUNTS}
host = {c: [] for c in COUNTS}
with NdtMatcher2D(fixed_iterations=K) as m:
    m.set_target(tx, ty)
    if FUSED is not None:
        m.set_tuning("fused_begin", FUSED)
    if LANE_FORK is not None:
        m.set_tuning("lane_fork", LANE_FORK)
    for rep in range(REPEATS + 1):              # sample 0 is the warm-up
        for lanes in COUNTS:
            m.set_tuning(KNOB, lanes)
            t0 = time.perf_counter()
            for _ in range(CALLS):
                m.align_async(sx, sy, d["init"], producer_complete=True)
            t1 = time.perf_counter()
            r = m.finish()
            el = time.perf_counter() - t0
            if rep:
                us[lanes].append(1e6 * el / (CALLS * (K + 1)))
                host[lanes].append(1e6 * (t1 - t0) / CALLS)
for lanes in COUNTS:
    a = np.array(us[lanes])
    print(f"{KNOB} {lanes}: {np.median(a):.3f} us per launch (min {a.min():.3f}, max {a.max():.3f}, {REPEATS} samples of "
          f"{CALLS} alignments; time / {K + 1} launches) = {np.median(a) * (K + 1):.1f} us per alignment = "
          f"{K / (K + 1) / np.median(a) * 1e3:.1f}k iterations/s; host enqueue {np.median(host[lanes]):.1f} us per alignment; fused_begin {'default' if FUSED is None else FUSED}; "
          f"lane_fork {'default' if LANE_FORK is None else LANE_FORK}; "
          f"{os.environ.get('NDT_HIP_LIB', 'product library')}; pose {r.pose}")
