"""Two launch chains per handle: consecutive asynchronous fixed-iteration alignments overlap in pairs
(NDT_TUNE_ASYNC_LANES, csrc/ndt_host.hpp).  Every alignment must stay what it is on a one-lane handle, bit for bit,
whichever lane it lands on and whatever else happens on the handle between the calls.

Shapes: the smallest at which the k_iterate graphs run - a 20 000-point target, 5 000-point scans (the short-scan
kernel ends at 4 096 points), 6 iterations.  The scans are different samplings of the target's scene, each with its
own initial pose."""
import numpy as np
import pytest

from gtsam_ndt_amd import synth

pytestmark = pytest.mark.gpu

K = 6
N_SCAN = 5000
L_ROOM = 50.0
TRUE_POSE = (0.10, -0.08, 0.01)


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


def _dev(scan):
    import torch
    return tuple(torch.from_numpy(a).cuda() for a in scan)


def _matcher(lanes, **tuning):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
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
        return [m.align(*s, p) for s, p in zip(dev_scans, world["inits"])]


def _run(m, dev_scans, inits, order):
    for k in order:
        m.align_async(*dev_scans[k], inits[k], producer_complete=True)
    return m.finish()


def test_every_lane_returns_the_one_lane_result(gpu_lib, world, dev_scans, want):
    """Sequences of 1..4 calls (lengths 2 and 4 end on lane 1, 1 and 3 on lane 0), the length-4 one three times."""
    assert len({w.pose for w in want}) == 4            # four different alignments: a mixed-up lane would show
    with _matcher(2) as m:
        m.set_target(world["tx"], world["ty"])
        for length in (1, 2, 3, 4, 4, 4):
            _same(_run(m, dev_scans, world["inits"], range(length)), want[length - 1])
        # a sequence whose last call is not the last scan: the pairing follows the calls, not the scans
        _same(_run(m, dev_scans, world["inits"], (3, 2, 1, 0, 1)), want[1])


def test_mixed_size_classes_in_flight(gpu_lib, world, dev_scans):
    """One call on 256-thread workgroups and one on 1024-thread ones (wide threshold lowered to 6 000 points) in flight
    together, in both orders."""
    import torch
    small, wide = dev_scans[0], _dev(world["wide_scan"])
    torch.cuda.synchronize()
    p0, p1 = world["inits"][1], world["inits"][2]
    with _matcher(1, wide_threshold=6000) as ref, _matcher(2, wide_threshold=6000) as m:
        ref.set_target(world["tx"], world["ty"])
        m.set_target(world["tx"], world["ty"])
        want_small, want_wide = ref.align(*small, p0), ref.align(*wide, p1)
        m.align_async(*small, p0, producer_complete=True)
        m.align_async(*wide, p1, producer_complete=True)
        _same(m.finish(), want_wide)
        m.align_async(*wide, p1, producer_complete=True)
        m.align_async(*small, p0, producer_complete=True)
        _same(m.finish(), want_small)


@pytest.mark.parametrize("change", ["set_target", "add_target_points"])
def test_second_call_sees_the_grid_changed_between_the_calls(gpu_lib, world, dev_scans, change):
    def change_grid(m):
        if change == "set_target":
            m.set_target(world["tx2"], world["ty2"])
        else:
            m.add_target_points(world["ex"], world["ey"])

    with _matcher(1) as ref:
        ref.set_target(world["tx"], world["ty"])
        before = ref.align(*dev_scans[1], world["inits"][1])
        change_grid(ref)
        after = ref.align(*dev_scans[1], world["inits"][1])
    assert before.pose != after.pose                    # the change is visible in the result
    with _matcher(2) as m:
        m.set_target(world["tx"], world["ty"])
        m.align_async(*dev_scans[0], world["inits"][0], producer_complete=True)
        change_grid(m)
        m.align_async(*dev_scans[1], world["inits"][1], producer_complete=True)
        _same(m.finish(), after)
        # and with the change behind a complete pair: the next pair forks behind it
        m.set_target(world["tx"], world["ty"])
        _run(m, dev_scans, world["inits"], (0, 1))
        change_grid(m)
        _same(_run(m, dev_scans, world["inits"], (0, 1)), after)


def test_lane_1_waits_for_the_producer_of_its_scan(gpu_lib, world, dev_scans, want):
    """The second call of a pair reads a scan that a side stream fills behind a long matrix product; no host
    synchronisation between producing and aligning it."""
    import torch
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    sx, sy = dev_scans[1]
    torch.cuda.synchronize()
    with _matcher(2) as m:
        m.set_target(world["tx"], world["ty"])
        with torch.cuda.stream(side):
            late_x = torch.full_like(sx, float("nan"))
            late_y = torch.full_like(sy, float("nan"))
            side.synchronize()
            b = a
            for _ in range(8):
                b = b @ a                                # tens of milliseconds on the side stream ...
            late_x.copy_(sx)                             # ... before the scan is there
            late_y.copy_(sy)
            m.align_async(*dev_scans[0], world["inits"][0], producer_complete=True)
            m.align_async(late_x, late_y, world["inits"][1])          # orders the handle behind `side`
        got = m.finish()
    _same(got, want[1])


def test_other_calls_between_and_after_a_pair(gpu_lib, world, dev_scans, want):
    """A multi-scan call behind a lane-1 call that was not finished: both are right, and finish() still returns the
    lane-1 alignment.  An evaluation in the middle of a pair starts the pairing over."""
    with _matcher(1) as ref:
        ref.set_target(world["tx"], world["ty"])
        want_multi = ref.align_multi_scan(dev_scans[2:4], world["inits"][2:4])
        want_eval = ref.evaluate(*dev_scans[3], world["inits"][3])
    with _matcher(2) as m:
        m.set_target(world["tx"], world["ty"])
        m.align_async(*dev_scans[0], world["inits"][0], producer_complete=True)
        m.align_async(*dev_scans[1], world["inits"][1], producer_complete=True)       # lane 1
        got_multi = m.align_multi_scan(dev_scans[2:4], world["inits"][2:4])
        _same(m.finish(), want[1])
        for g, w in zip(got_multi, want_multi):
            _same(g, w)
        m.align_async(*dev_scans[0], world["inits"][0], producer_complete=True)
        got_eval = m.evaluate(*dev_scans[3], world["inits"][3])
        assert np.array_equal(got_eval[0], want_eval[0]) and np.array_equal(got_eval[1], want_eval[1])
        assert got_eval[2:] == want_eval[2:]
        _same(_run(m, dev_scans, world["inits"], (1, 2)), want[2])


def test_the_knob(gpu_lib, world, dev_scans, want):
    from gtsam_ndt_amd import _lib as L
    with _matcher(1) as m:
        m.set_target(world["tx"], world["ty"])
        _same(_run(m, dev_scans, world["inits"], range(4)), want[3])
        for bad in (0, 3):
            with pytest.raises(L.NdtError) as e:
                m.set_tuning("async_lanes", bad)
            assert e.value.code == L.NDT_ERR_INVALID_ARG
        m.set_tuning("async_lanes", 2)
        _same(_run(m, dev_scans, world["inits"], range(4)), want[3])
