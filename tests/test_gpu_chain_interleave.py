"""Another call made on a handle while an asynchronous alignment is in flight on it: the sequence that
tests/test_gpu_handle_life.py leaves out (there every run of align_async calls is finished before the next step).
include/ndt_hip.h promises that such a call "finishes a loop in flight first"; the one record of what is in flight
(csrc/ndt_host.hpp: ChainFlight), which both handles share, is what keeps that promise.

For each in-flight state
  2d_fixed      fixed_iterations = 3, two align_async calls of 5 000-point device scans: lanes 0 and 1 hold chains
  2d_small      one align_async of a 1 000-point scan: a k_align_small launch in flight
  2d_converged  fixed_iterations = 0, one align_async of 5 000 points: a chunk run in flight
  3d_fixed      fixed_iterations = 3, one align_async of 5 000 points: the chain and the copy of its state are queued
  3d_converged  one align_async of 5 000 points: a chunk run in flight
each follower call (evaluate, align on device arrays, align on host arrays, align_trace, align_multi_start with 2 starts,
align_map with the busy handle as target, align_map with the busy handle as source; one pair excepted: CASES) answers, byte
for byte, what the same
call answers on a fresh handle that loaded the same map and has nothing in flight (bitwise equality between two handles is
what the contract promises for these families: tests/test_gpu_handle_life.py).  Afterwards finish() on the busy handle
returns without error; the header does not define its value there, so nothing more is asserted of it.  The in-flight
scans' arrays stay alive until that finish().

The fresh handle's answers depend on the dimension, the parameters and the follower alone: they are computed once each
and shared between the in-flight states.  Targets hold 3 000 points; a case takes a few milliseconds."""
import numpy as np
import pytest

import handle_life as HL
from test_gpu_handle_life import _assert_same, _cols, _dev, _flat, _matcher

pytestmark = pytest.mark.gpu

# state -> (dimension, parameters, sizes of the scans put in flight)
STATES = {
    "2d_fixed": (2, {"fixed_iterations": 3}, (5000, 5000)),
    "2d_small": (2, {}, (1000,)),
    "2d_converged": (2, {}, (5000,)),
    "3d_fixed": (3, {"fixed_iterations": 3}, (5000,)),
    "3d_converged": (3, {}, (5000,)),
}
FOLLOWERS = ("evaluate", "align_dev", "align_host", "align_trace", "multi_start", "align_map_target", "align_map_source")

_inputs, _blobs, _wanted = {}, {}, {}


def _scene(dim):
    """The inputs of one dimension (cached, left unchanged): the two target clouds, the scans to put in flight, the
    followers' scans, starts and map poses."""
    if dim not in _inputs:
        g = HL._Gen(dim, 77)
        clouds = [g.cloud(3000, size=24.0), g.cloud(3000, size=24.0)]
        for who in (0, 1):
            g.set_scene(who, clouds[who])
        big, _, big_init = g.scan(0, 4097)
        small, _, small_init = g.scan(0, 1000)
        _inputs[dim] = dict(
            clouds=clouds, flight=[g.scan(0, n) for n in (5000, 5000, 1000)], big=big, big_init=big_init, small=small,
            small_init=small_init, starts=g.starts(big_init, 2), pose_target=g.map_pose(0), pose_source=g.map_pose(1))
    return _inputs[dim]


def _loaded(dim, params, who):
    """A fresh handle of these parameters holding cloud `who` (the blob of one set_target, saved once per dimension)."""
    if (dim, who) not in _blobs:
        with _matcher(dim) as m:
            m.set_target(*_cols(_scene(dim)["clouds"][who]))
            _blobs[(dim, who)] = m.save_map()
    m = _matcher(dim, **params)
    m.load_map(_blobs[(dim, who)])
    return m


def _follow(name, dim, h, partner):
    """The follower call `name` on h (holding cloud 0), with `partner` (holding cloud 1) for the map-to-map calls."""
    s = _scene(dim)
    if name == "evaluate":
        return h.evaluate(*_dev(s["big"]), tuple(s["big_init"]))
    if name == "align_dev":
        return h.align(*_dev(s["big"]), tuple(s["big_init"]))
    if name == "align_host":
        return h.align(*_cols(s["small"]), tuple(s["small_init"]))
    if name == "align_trace":
        return h.align_trace(*_cols(s["small"]), tuple(s["small_init"]))
    if name == "multi_start":
        return h.align_multi_start(*_dev(s["big"]), s["starts"])
    if name == "align_map_target":
        return h.align_map(partner, tuple(s["pose_target"]))
    if name == "align_map_source":
        return partner.align_map(h, tuple(s["pose_source"]))
    raise KeyError(name)


def _want(name, dim, params):
    key = (name, dim, tuple(sorted(params.items())))
    if key not in _wanted:
        with _loaded(dim, params, 0) as fresh, _loaded(dim, params, 1) as partner:
            _wanted[key] = _flat(_follow(name, dim, fresh, partner))
    return _wanted[key]


# One pair is left out: align_map with the busy handle as target behind 2d_fixed.  Before the in-flight record was one
# struct, the 2D map-to-map chain recorded the parity of its final state but not its lane, so behind a chain on lane 1 the
# call returned lane 1's state: there was no behaviour to preserve, and this file pins only what was.
CASES = [(s, f) for s in STATES for f in FOLLOWERS if (s, f) != ("2d_fixed", "align_map_target")]


@pytest.mark.parametrize("state,follower", CASES)
def test_a_call_behind_an_alignment_in_flight(gpu_lib, state, follower):
    dim, params, sizes = STATES[state]
    want = _want(follower, dim, params)
    by_size = {5000: [0, 1], 1000: [2]}
    with _loaded(dim, params, 0) as busy, _loaded(dim, params, 1) as partner:
        kept = []                                                   # the in-flight scans' arrays, alive until finish()
        for n in sizes:
            scan, _, init = _scene(dim)["flight"][by_size[n].pop(0)]
            kept.append(_dev(scan))
            busy.align_async(*kept[-1], tuple(init))
        got = _flat(_follow(follower, dim, busy, partner))
        _assert_same(got, want, f"{follower} behind {state}")
        busy.finish()                                               # returns without error; its value is not defined here
        del kept
