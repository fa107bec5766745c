"""Up to four launch chains per handle: consecutive asynchronous fixed-iteration alignments go round them
(NDT_TUNE_ASYNC_CHAINS, csrc/ndt_host.hpp).  Every alignment must stay what align() returns on a one-chain handle, bit
for bit, whichever chain it lands on and whatever else happens on the handle between the calls.

Shapes: those of test_gpu_async_lanes.py, the smallest at which the k_iterate graphs run - a 20 000-point target,
5 000-point scans (the short-scan kernel ends at 4 096 points), 6 iterations.  Nine scans, different samplings of the
target's scene, each with its own initial pose: a sequence of 2 N + 1 calls at N = 4 ends on a scan of its own."""
import numpy as np
import pytest

from gtsam_ndt_amd import synth

pytestmark = pytest.mark.gpu

K = 6
N_SCAN = 5000
N_SCANS = 9
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

    scans = [scan(900 + k) for k in range(N_SCANS)]
    inits = [(0.01 * k, -0.008 * k, 0.001 * k) for k in range(N_SCANS)]
    tx2, ty2 = synth.sample_scene(scene, 20000, seed=777, sigma=synth.SIGMA)
    ex, ey = synth.sample_scene(scene, 3000, seed=778, sigma=synth.SIGMA)
    return {"tx": d["tx"], "ty": d["ty"], "tx2": f(tx2), "ty2": f(ty2), "ex": f(ex), "ey": f(ey),
            "scans": scans, "inits": inits, "wide_scan": scan(600, 6000)}


def _dev(scan):
    import torch
    return tuple(torch.from_numpy(a).cuda() for a in scan)


def _matcher(chains, **tuning):
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    return NdtMatcher2D(fixed_iterations=K, tuning={"async_chains": chains, **tuning})


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
    """What a one-chain handle returns from align() for every scan from its initial pose."""
    with _matcher(1) as m:
        m.set_target(world["tx"], world["ty"])
        w = [m.align(*s, p) for s, p in zip(dev_scans, world["inits"])]
    assert len({r.pose for r in w}) == N_SCANS             # nine different alignments: a mixed-up chain would show
    return w


def _run(m, dev_scans, inits, order):
    for k in order:
        m.align_async(*dev_scans[k], inits[k], producer_complete=True)
    return m.finish()


@pytest.mark.parametrize("chains", [1, 2, 3, 4])
def test_every_chain_returns_the_one_chain_result(gpu_lib, world, dev_scans, want, chains):
    """Sequences of 1 .. 2 N + 1 calls: the last call lands on every chain, in the first round and in a later one.  The
    longest three times over on the same handle."""
    longest = 2 * chains + 1
    with _matcher(chains) as m:
        m.set_target(world["tx"], world["ty"])
        for length in (*range(1, longest + 1), longest, longest):
            _same(_run(m, dev_scans, world["inits"], range(length)), want[length - 1])
        # a sequence whose last call is not the last scan: the rotation follows the calls, not the scans
        _same(_run(m, dev_scans, world["inits"], (8, 7, 6, 5, 4, 3)), want[3])


def test_a_new_handle_runs_more_than_two_chains(gpu_lib, world, dev_scans, want):
    """The default count: whatever it is, the results are the one-chain handle's."""
    from gtsam_ndt_amd.matcher import NdtMatcher2D
    with NdtMatcher2D(fixed_iterations=K) as m:
        m.set_target(world["tx"], world["ty"])
        for length in (9, 5, 9):
            _same(_run(m, dev_scans, world["inits"], range(length)), want[length - 1])


@pytest.mark.parametrize("change", ["set_target", "add_target_points"])
def test_the_next_call_sees_the_grid_changed_in_any_gap_of_a_round(gpu_lib, world, dev_scans, change):
    def change_grid(m):
        if change == "set_target":
            m.set_target(world["tx2"], world["ty2"])
        else:
            m.add_target_points(world["ex"], world["ey"])

    with _matcher(1) as ref:
        ref.set_target(world["tx"], world["ty"])
        before = [ref.align(*dev_scans[k], world["inits"][k]) for k in range(5)]
        change_grid(ref)
        after = [ref.align(*dev_scans[k], world["inits"][k]) for k in range(5)]
    assert all(b.pose != a.pose for b, a in zip(before, after))          # the change is visible in every result
    with _matcher(4) as m:
        for gap in range(1, 5):
            # `gap` calls of a round on the old grid (the last of them on chain gap - 1), the change, then a whole round
            # on the new grid: its calls land on chains 0 .. 3 again, each behind the change
            m.set_target(world["tx"], world["ty"])
            _same(_run(m, dev_scans, world["inits"], range(gap)), before[gap - 1])
            for k in range(gap):
                m.align_async(*dev_scans[k], world["inits"][k], producer_complete=True)
            change_grid(m)
            for length in range(1, 5):
                _same(_run(m, dev_scans, world["inits"], range(length)), after[length - 1])
        # the change in the gaps of a round in steady state, without a finish() before it: the call after it is the
        # first of a new round, and the calls behind that one reach chains 1, 2 and 3 with the new grid
        for gap in range(1, 5):
            m.set_target(world["tx"], world["ty"])
            for k in range(4 + gap):
                m.align_async(*dev_scans[k % 5], world["inits"][k % 5], producer_complete=True)
            change_grid(m)
            for k in range(gap):
                m.align_async(*dev_scans[k], world["inits"][k], producer_complete=True)
            _same(m.finish(), after[gap - 1])


@pytest.mark.parametrize("chain", [2, 3])
def test_a_further_chain_waits_for_the_producer_of_its_scan(gpu_lib, world, dev_scans, want, chain):
    """The call that lands on chain 2 (or 3) reads a scan that a side stream fills behind a long matrix product; no host
    synchronisation between producing and aligning it."""
    import torch
    side = torch.cuda.Stream()
    a = torch.randn(4096, 4096, device="cuda")
    sx, sy = dev_scans[chain]
    torch.cuda.synchronize()
    with _matcher(4) as m:
        m.set_target(world["tx"], world["ty"])
        # steady state first: no chain forks any more, so only the producer's event can order the late scan
        _run(m, dev_scans, world["inits"], range(8))
        with torch.cuda.stream(side):
            late_x = torch.full_like(sx, float("nan"))
            late_y = torch.full_like(sy, float("nan"))
            side.synchronize()
            b = a
            for _ in range(8):
                b = b @ a                                # tens of milliseconds on the side stream ...
            late_x.copy_(sx)                             # ... before the scan is there
            late_y.copy_(sy)
            for k in range(chain):
                m.align_async(*dev_scans[k], world["inits"][k], producer_complete=True)
            m.align_async(late_x, late_y, world["inits"][chain])          # orders the handle behind `side`
        got = m.finish()
    _same(got, want[chain])


def test_other_calls_in_the_middle_of_a_round(gpu_lib, world, dev_scans, want):
    """A multi-scan call behind a chain-2 call that was not finished: both are right, and finish() still returns the
    chain-2 alignment.  An evaluation in the middle of a round starts the rotation over."""
    with _matcher(1) as ref:
        ref.set_target(world["tx"], world["ty"])
        want_multi = ref.align_multi_scan(dev_scans[3:5], world["inits"][3:5])
        want_eval = ref.evaluate(*dev_scans[5], world["inits"][5])
    with _matcher(4) as m:
        m.set_target(world["tx"], world["ty"])
        for k in range(3):
            m.align_async(*dev_scans[k], world["inits"][k], producer_complete=True)        # the last one on chain 2
        got_multi = m.align_multi_scan(dev_scans[3:5], world["inits"][3:5])
        _same(m.finish(), want[2])
        for g, w in zip(got_multi, want_multi):
            _same(g, w)
        for k in range(2):
            m.align_async(*dev_scans[k], world["inits"][k], producer_complete=True)
        got_eval = m.evaluate(*dev_scans[5], world["inits"][5])
        assert np.array_equal(got_eval[0], want_eval[0]) and np.array_equal(got_eval[1], want_eval[1])
        assert got_eval[2:] == want_eval[2:]
        _same(_run(m, dev_scans, world["inits"], (1, 2, 3, 4)), want[4])


def test_mixed_size_classes_in_flight(gpu_lib, world, dev_scans):
    """One call on 1024-thread workgroups (wide threshold lowered to 6 000 points) among 256-thread ones, across three
    chains, the wide one on each of them in turn."""
    import torch
    wide = _dev(world["wide_scan"])
    torch.cuda.synchronize()
    inits = world["inits"]
    with _matcher(1, wide_threshold=6000) as ref, _matcher(3, wide_threshold=6000) as m:
        ref.set_target(world["tx"], world["ty"])
        m.set_target(world["tx"], world["ty"])
        want_small, want_wide = ref.align(*dev_scans[1], inits[1]), ref.align(*wide, inits[2])
        for at in range(3):
            for k in range(3):
                m.align_async(*(wide if k == at else dev_scans[0]), inits[2] if k == at else inits[0], producer_complete=True)
            m.align_async(*dev_scans[1], inits[1], producer_complete=True)
            _same(m.finish(), want_small)
            for k in range(at + 1):
                m.align_async(*(wide if k == at else dev_scans[0]), inits[2] if k == at else inits[0], producer_complete=True)
            _same(m.finish(), want_wide)


def test_fork_at_every_round(gpu_lib, world, dev_scans, want):
    with _matcher(4, lane_fork=1) as m:
        m.set_target(world["tx"], world["ty"])
        for length in (9, 1, 2, 3, 4, 9):
            _same(_run(m, dev_scans, world["inits"], range(length)), want[length - 1])


def test_switching_the_count_between_sequences(gpu_lib, world, dev_scans, want):
    with _matcher(4) as m:
        m.set_target(world["tx"], world["ty"])
        _same(_run(m, dev_scans, world["inits"], range(7)), want[6])
        for chains in (2, 3):
            m.set_tuning("async_chains", chains)
            for length in (2 * chains + 1, chains, chains + 1):
                _same(_run(m, dev_scans, world["inits"], range(length)), want[length - 1])


def test_the_knobs(gpu_lib, world, dev_scans, want):
    from gtsam_ndt_amd import _lib as L
    with _matcher(1) as m:
        m.set_target(world["tx"], world["ty"])
        for knob, bad in (("async_chains", 0), ("async_chains", 5), ("async_lanes", 0), ("async_lanes", 3)):
            with pytest.raises(L.NdtError) as e:
                m.set_tuning(knob, bad)
            assert e.value.code == L.NDT_ERR_INVALID_ARG
        _same(_run(m, dev_scans, world["inits"], range(4)), want[3])           # a refused value changes nothing
        for knob, value in (("async_chains", 4), ("async_lanes", 2), ("async_chains", 3), ("async_lanes", 1)):
            m.set_tuning(knob, value)
            _same(_run(m, dev_scans, world["inits"], range(5)), want[4])
