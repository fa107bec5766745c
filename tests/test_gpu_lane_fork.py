"""Lane 1 of a handle forks from the handle's stream only where something other than an alternating asynchronous
alignment precedes a pair (NDT_TUNE_LANE_FORK = 0, the default; csrc/ndt_host.hpp: lane_step), and runs its chains back
to back otherwise.  Every alignment must stay what it is on a one-lane handle, bit for bit, whichever lane it lands on,
however long ago lane 1 last waited for the handle's stream and whatever else happens on the handle in between - under
both values of the knob (1: a fork at every pair).

Shapes as tests/test_gpu_async_lanes.py, the smallest at which the k_iterate graphs run: a 20 000-point target,
5 000-point scans (the short-scan kernel ends at 4 096 points), 6 iterations."""
import numpy as np
import pytest

from gtsam_ndt_amd import synth

pytestmark = pytest.mark.gpu

K = 6
N_SCAN = 5000
L_ROOM = 50.0
TRUE_POSE = (0.10, -0.08, 0.01)
FORKS = (0, 1)


@pytest.fixture(scope="module")
def world():
    """Target clouds and scans on the host, made once: the scene is the one make_pair(2) samples its target from."""
    d = synth.make_pair(2, n_tgt=20000, n_src=N_SCAN)
    scene = synth.room_scene(2, L_ROOM, -0.5 * L_ROOM, -0.5 * L_ROOM)
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)

    def scan(seed, n=N_SCAN):
        x, y = synth.sample_scene(scene, n, seed=seed, sigma=synth.SIGMA)
        x, y = synth.to_source_frame(x, y, TRUE_POSE)
        return f(x), f(y)

    scans = [scan(500 + k) for k in range(4)]
    inits = [(0.02 * k, -0.015 * k, 0.002 * k) for k in range(4)]
    tx2, ty2 = synth.sample_scene(scene, 20000, seed=777, sigma=synth.SIGMA)
    ex, ey = synth.sample_scene(scene, 3000, seed=778, sigma=synth.SIGMA)
    return {"tx": d["tx"], "ty": d["ty"], "tx2": f(tx2), "ty2": f(ty2), "ex": f(ex), "ey": f(ey),
            "scans": scans, "inits": inits, "wide_scan": scan(600, 6000)}


def _dev(arrays):
    import torch
    return tuple(torch.from_numpy(a).cuda() for a in arrays)


def _matcher(lanes, fork=None, **tuning):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    if fork is not None:
        tuning["lane_fork"] = fork
    return NdtMatcher2D(fixed_iterations=K, tuning={"async_lanes": lanes, **tuning})


def _same(a, b):
    assert a.pose == b.pose and a.score == b.score and a.n_hit == b.n_hit
    assert a.iterations == b.iterations == K and a.status == b.status
    assert np.array_equal(a.H, b.H) and np.array_equal(a.g, b.g)


@pytest.fixture(scope="module")
def dev_scans(gpu_lib, world):
    import torch
    s = [_dev(sc) for sc in world["scans"]]
    torch.cuda.synchronize()
    return s


@pytest.fixture(scope="module")
def want(gpu_lib, world, dev_scans):
    """What a one-lane handle returns from align() for every scan from its initial pose."""
    with _matcher(1) as m:
        m.set_target(world["tx"], world["ty"])
        w = [m.align(*s, p) for s, p in zip(dev_scans, world["inits"])]
    assert len({r.pose for r in w}) == 4               # four different alignments: a mixed-up lane or scan would show
    return w


@pytest.fixture(scope="module")
def long_product(gpu_lib):
    """The operand of the matrix products that keep a stream busy for tens of milliseconds in front of a late write."""
    import torch
    a = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    return a


def _delay(a):
    """Tens of milliseconds of work on torch's current stream."""
    b = a
    for _ in range(8):
        b = b @ a
    return b


def _calls(m, dev_scans, inits, count, start=0):
    """`count` back-to-back asynchronous calls, scan (start + j) % 4 for call j; returns the index of the last scan."""
    k = start
    for j in range(count):
        k = (start + j) % 4
        m.align_async(*dev_scans[k], inits[k], producer_complete=True)
    return k


@pytest.mark.parametrize("fork", FORKS)
def test_long_runs_of_back_to_back_calls(gpu_lib, world, dev_scans, want, fork):
    """Runs of 1 to 9 calls on one handle: the last call lands on either lane, long after the only fork of the handle
    (finish() between the runs does not make lane 1 stale).  The 8-call run three times."""
    with _matcher(2, fork) as m:
        m.set_target(world["tx"], world["ty"])
        for length in (1, 2, 3, 4, 5, 6, 7, 8, 8, 8, 9):
            last = _calls(m, dev_scans, world["inits"], length)
            _same(m.finish(), want[last])
        # a run whose last call is not the scan its position suggests: the lanes follow the calls, not the scans
        last = _calls(m, dev_scans, world["inits"], 6, start=3)
        _same(m.finish(), want[last])


@pytest.mark.parametrize("fork", FORKS)
@pytest.mark.parametrize("change", ["set_target", "add_target_points"])
def test_grid_change_in_steady_state(gpu_lib, world, dev_scans, long_product, change, fork):
    """Four calls, a new grid, two calls: the lane-1 call behind the change sees the new grid.  The new points are
    written on a side stream behind a long matrix product, with no host synchronisation of the test's own.
    This pins the results around a grid change; it cannot catch a missing fork: set_target and add_target_points wait on
    the host for the build's counters, so the grid is complete (but for the small upload of the static context) before
    the next call is enqueued.  test_the_fork_behind_other_work_is_waited_for is the case that fails without the wait."""
    import torch

    def change_grid(m, late):
        x, y = _dev((world["tx2"], world["ty2"]) if change == "set_target" else (world["ex"], world["ey"]))
        torch.cuda.synchronize()
        if not late:
            return m.set_target(x, y) if change == "set_target" else m.add_target_points(x, y)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            lx, ly = torch.full_like(x, float("nan")), torch.full_like(y, float("nan"))
            side.synchronize()
            _delay(long_product)
            lx.copy_(x)
            ly.copy_(y)
            r = m.set_target(lx, ly) if change == "set_target" else m.add_target_points(lx, ly)
        return r

    with _matcher(1) as ref:
        ref.set_target(world["tx"], world["ty"])
        before = ref.align(*dev_scans[1], world["inits"][1])
        change_grid(ref, late=False)
        after = [ref.align(*dev_scans[k], world["inits"][k]) for k in (0, 1)]
    assert before.pose != after[1].pose                 # the change is visible in the result
    with _matcher(2, fork) as m:
        m.set_target(world["tx"], world["ty"])
        _calls(m, dev_scans, world["inits"], 4)
        change_grid(m, late=True)
        _calls(m, dev_scans, world["inits"], 2)          # lane 0, lane 1
        _same(m.finish(), after[1])
        # the pair after that forks no more, and the lane-0 call of a third one is right as well
        _calls(m, dev_scans, world["inits"], 2)
        _same(m.finish(), after[1])
        _calls(m, dev_scans, world["inits"], 1)
        _same(m.finish(), after[0])


@pytest.mark.parametrize("fork", FORKS)
@pytest.mark.parametrize("producer", ["side", "own"])
def test_sixth_call_waits_for_the_late_producer_of_its_scan(gpu_lib, world, dev_scans, want, long_product, producer, fork):
    """Five calls, then a lane-1 call whose scan is written behind a long matrix product - on a side stream, or on the
    handle's own stream (the caller's work on ndt2d_stream) - and passed without producer_complete: align_async orders
    the handle, lane 1 included, behind torch's current stream.  No host synchronisation between writing and aligning."""
    import torch
    sx, sy = dev_scans[1]
    with _matcher(2, fork) as m:
        m.set_target(world["tx"], world["ty"])
        stream = torch.cuda.Stream() if producer == "side" else torch.cuda.ExternalStream(m.stream)
        late_x, late_y = torch.full_like(sx, float("nan")), torch.full_like(sy, float("nan"))
        torch.cuda.synchronize()
        _calls(m, dev_scans, world["inits"], 5)
        with torch.cuda.stream(stream):
            busy = _delay(long_product)                  # tens of milliseconds on the producer's stream ...
            late_x.copy_(sx)                             # ... before the scan is there
            late_y.copy_(sy)
            m.align_async(late_x, late_y, world["inits"][1])
        got = m.finish()
        del busy
    _same(got, want[1])


@pytest.mark.parametrize("fork", FORKS)
def test_the_fork_behind_other_work_is_waited_for(gpu_lib, world, dev_scans, want, long_product, fork):
    """The wiring of the rule into the streams (lane_step's mark -> the fork event recorded, wait -> lane 1 waits for
    it), with work on the handle's stream that really is in flight when the lane-1 call is enqueued.  No entry point of
    the library leaves such work behind (they end in a host wait), so the test puts it there: a long matrix product and
    then the scan of the lane-1 call, written on the handle's own stream.  A tuning change (an `other` call) follows,
    so the next pair forks: its lane-1 call is behind everything that preceded its lane-0 partner on the handle's
    stream, the scan included, although it is passed as complete.  Without the record or the wait it reads NaN points.
    (A check of the mechanism from inside; a caller orders such a scan with ndt2d_wait_stream.)"""
    import torch
    sx, sy = dev_scans[1]
    with _matcher(2, fork) as m:
        m.set_target(world["tx"], world["ty"])
        late_x, late_y = torch.full_like(sx, float("nan")), torch.full_like(sy, float("nan"))
        torch.cuda.synchronize()
        _calls(m, dev_scans, world["inits"], 4)          # steady state: lane 1 has long stopped waiting for forks
        with torch.cuda.stream(torch.cuda.ExternalStream(m.stream)):
            busy = _delay(long_product)
            late_x.copy_(sx)
            late_y.copy_(sy)
        m.set_tuning("lane_fork", fork)                  # the `other` call: lane 1 is stale, nothing is enqueued
        m.align_async(*dev_scans[0], world["inits"][0], producer_complete=True)       # lane 0: records the fork
        m.align_async(late_x, late_y, world["inits"][1], producer_complete=True)      # lane 1: waits for it
        got = m.finish()
        del busy
    _same(got, want[1])


@pytest.mark.parametrize("fork", FORKS)
@pytest.mark.parametrize("between", ["evaluate", "align", "finish", "async_lanes", "lane_fork"])
def test_other_traffic_in_steady_state(gpu_lib, world, dev_scans, want, between, fork):
    """Steady state, something else on the handle, two more calls: both the call in between and the lane-1 call behind
    it are what a one-lane handle returns."""
    inits = world["inits"]
    with _matcher(1) as ref:
        ref.set_target(world["tx"], world["ty"])
        want_eval = ref.evaluate(*dev_scans[3], inits[3])
    with _matcher(2, fork) as m:
        m.set_target(world["tx"], world["ty"])
        if between == "evaluate":
            _calls(m, dev_scans, inits, 4)
            got = m.evaluate(*dev_scans[3], inits[3])
            assert np.array_equal(got[0], want_eval[0]) and np.array_equal(got[1], want_eval[1])
            assert got[2:] == want_eval[2:]
        elif between == "align":
            _calls(m, dev_scans, inits, 4)
            _same(m.align(*dev_scans[2], inits[2]), want[2])
        elif between == "finish":
            last = _calls(m, dev_scans, inits, 5)         # ends inside a pair: the next call is a lane-0 call again
            _same(m.finish(), want[last])
        elif between == "async_lanes":
            _calls(m, dev_scans, inits, 4)
            m.set_tuning("async_lanes", 1)
            last = _calls(m, dev_scans, inits, 3)
            m.set_tuning("async_lanes", 2)
            _same(m.finish(), want[last])
        else:
            _calls(m, dev_scans, inits, 4)
            m.set_tuning("lane_fork", 1 - fork)
            last = _calls(m, dev_scans, inits, 4)
            m.set_tuning("lane_fork", fork)
            _same(m.finish(), want[last])
        last = _calls(m, dev_scans, inits, 2)
        _same(m.finish(), want[last])
        last = _calls(m, dev_scans, inits, 3, start=1)
        _same(m.finish(), want[last])


@pytest.mark.parametrize("fork", FORKS)
def test_mixed_size_classes_in_steady_state(gpu_lib, world, dev_scans, fork):
    """Calls on 256-thread workgroups and on 1024-thread ones (wide threshold lowered to 6 000 points) alternate on the
    free-running lanes, each size on either lane."""
    import torch
    small, wide = dev_scans[0], _dev(world["wide_scan"])
    torch.cuda.synchronize()
    p0, p1 = world["inits"][1], world["inits"][2]
    with _matcher(1, wide_threshold=6000) as ref, _matcher(2, fork, wide_threshold=6000) as m:
        ref.set_target(world["tx"], world["ty"])
        m.set_target(world["tx"], world["ty"])
        want_small, want_wide = ref.align(*small, p0), ref.align(*wide, p1)
        assert want_small.pose != want_wide.pose
        for order in ("swswsw", "swsws", "wwsswws", "sswwssww"):
            for c in order:
                m.align_async(*(small if c == "s" else wide), p0 if c == "s" else p1, producer_complete=True)
            _same(m.finish(), want_small if order[-1] == "s" else want_wide)


def test_the_knob(gpu_lib, world, dev_scans, want):
    """0 is the default; other values than 0 and 1 are refused and leave the knob as it was; 2D handles only."""
    from gtsam_ndt_amd import _lib as L
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    assert L.TUNING["lane_fork"] == 14
    with _matcher(2) as m:
        m.set_target(world["tx"], world["ty"])
        for bad in (-1, 2):
            with pytest.raises(L.NdtError) as e:
                m.set_tuning("lane_fork", bad)
            assert e.value.code == L.NDT_ERR_INVALID_ARG
        last = _calls(m, dev_scans, world["inits"], 4)
        _same(m.finish(), want[last])
    with NdtMatcher3D() as m3:
        assert L.load().ndt3d_set_tuning(m3._h, L.TUNING["lane_fork"], 0) == L.NDT_ERR_INVALID_ARG
