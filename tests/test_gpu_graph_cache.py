"""One handle driven past the sixteen slots of its launch-chain graph cache (ChainGraphCache, csrc/ndt_host.hpp): eviction is
ordinary use.  A cached graph bakes device pointers and launch shapes and is found by an integer key alone, so a key that
forgot a launch dimension, an executable destroyed while a chain still replays it, or a pointer that outlives its slot would
show as wrong bits.  Every result here is compared, as bytes, with the same call on a FRESH handle that loaded the same map
and holds one graph.  fixed_iterations = 3 (30 in the lane test), a 20 000-point target, 5 000-point device scans - above the
4096-point short-scan limit and below wide_threshold, so every chain is a graph of 256-thread workgroups.

THE KEYS (a slot matches on launches, blocks = the first kernel's grid.x, mode, lane, first_parity):

2D, multi_align (ndt2d_api.hip): mode = 0x10000 | 0x20000 (multi_scan) | 0x40000 (split) | nh << 5 | subsets << 8 | hessian.
  Fused chain (m < split_from = 12): nh = 1 for m <= 6, else 2; subsets = ceil(m / nh).  m = 1..11 therefore gives NINE keys
  per call kind, not eleven: (nh 1; 1..6 subsets), (2; 4) for m = 7 and 8, (2; 5) for m = 9 and 10, (2; 6) for m = 11.
  Split chain (m >= 12): mg = 16, 32, 64 slots for m = 12, 17, 33, in the key as mg << 8 | mg << 20, and as blocks.
  align: begin_align -> run_chain_tail (ndt_chain_host.hpp), launches = K = 3 behind k_iterate_first, mode = hessian, lane 0,
  first_parity 1.
  evaluate: the same with launches = 1.  align_trace: plain launches, no graph.
  test_multi_start_shapes_2d walks S1..S11, C1..C11 (start, scan), the six split keys, align, evaluate: 26 distinct keys.
  Behind the last use of S11 come 9 + 6 + 2 = 17 other keys, behind every earlier S more: each of m = 11..1 in the last
  pass finds its graph evicted and rebuilds it (test_the_key_model_says_every_reuse_is_a_rebuild replays this on an LRU
  of 16).

2D / 3D, align_map_pair (ndt_map_host.hpp) -> run_chain_tail: mode = kMapGraphKey | hessian, launches = K + 1 = 4,
  blocks = min(ceil(n_comp / 256), 256) of the SOURCE.  Twenty sources with at least 17 distinct blocks (asserted from
  components()), aligned twice round: 19 other sources lie between two uses of one key.  run_map_multi_graph: mode =
  kMapMultiGraphKey | pow2(max blocks of the starts) << 8 | hessian, blocks = pow2(m): m = 2, 5, 9, 17 add keys in between.

2D lanes (begin_align): the key carries the lane, so after the cache was filled with the 18 fused multi keys, a run of r
  back-to-back align_async calls needs r new keys (lane 0..r-1, launches 30); the call on lane k evicts while the chains of
  lanes 0..k-1 are queued.  ChainGraphCache::victim drains the handle's stream and the lane streams first.

3D, multi_align3 (ndt3d_api.hpp): two-kernel chains, mode = 0x100000 | mg << 8 | graph_mode3 (0x10 with neighbourhood 7),
  blocks = mg = 1, 2, 4, ..., 64; start and scan calls share keys.  align / evaluate: run_chain_tail, launches 3 / 1, mode =
  graph_mode3.  m = 1, 2, 3, 5, 9, 17, 33 under both neighbourhoods, with align and evaluate: 18 keys per pass, so the
  second pass finds every graph evicted.  The 3D handle has one launch chain: its asynchronous calls follow one another on
  the handle's stream, and the first of a run evicts while nothing of that run is queued yet.

Between align_async and align_finish only further align_async calls are made.  The header says of another call in between
only that "any other call on the handle finishes a loop in flight first"; it does not say what align_finish returns
afterwards, so that sequence is left out (tests/test_gpu_chain_interleave.py pins the call in between).

Wall time on one MI355X: test_multi_start_shapes_2d 0.39 s, test_multi_start_shapes_3d 0.13 s, test_map_to_map_shapes 0.26 s
(2D) and 0.16 s (3D), test_eviction_while_lanes_are_busy_2d 0.08 s, test_eviction_in_front_of_async_runs_3d 0.08 s,
test_the_key_model_says_every_reuse_is_a_rebuild below 0.005 s; loading the library for the first test of the file 1.6 s."""
import numpy as np
import pytest

import handle_life as HL

pytestmark = pytest.mark.gpu

SLOTS = 16


# ---- the key model (a restatement of the code above, for the docstring's counts) -------------------------------------------
def multi_key_2d(m, shared):
    if m >= 12:
        mg = 1 << (m - 1).bit_length()
        return ("multi", shared, "split", mg)
    nh = 1 if m <= 6 else 2
    return ("multi", shared, nh, -(-m // nh))


def walk_2d():
    """(call, key or None) in the order of test_multi_start_shapes_2d."""
    calls = [(("multi_start", m), multi_key_2d(m, True)) for m in range(1, 12)]
    calls += [(("multi_scan", m), multi_key_2d(m, False)) for m in range(1, 12)]
    calls += [(("multi_start", m), multi_key_2d(m, True)) for m in (12, 17, 33)]
    calls += [(("multi_scan", m), multi_key_2d(m, False)) for m in (12, 17, 33)]
    calls += [(("align", 0), ("align", 3)), (("evaluate", 0), ("align", 1)), (("align_trace", 0), None)]
    calls += [(("multi_start", m), multi_key_2d(m, True)) for m in range(11, 0, -1)]
    return calls


def walk_3d():
    calls = []
    for _ in range(2):
        for nb in (1, 7):
            calls.append((("neighbourhood", nb), None))
            for m in (1, 2, 3, 5, 9, 17, 33):
                calls.append((("multi_start" if m % 2 else "multi_scan", m), ("multi3", nb, 1 << (m - 1).bit_length())))
            calls += [(("align", 0), ("align3", nb, 3)), (("evaluate", 0), ("align3", nb, 1)), (("align_trace", 0), None)]
    return calls


def lru_misses(keys):
    """For each key of the sequence: was its graph absent from a least-recently-used cache of SLOTS entries?"""
    held, out = [], []
    for k in keys:
        out.append(k not in held)
        if k in held:
            held.remove(k)
        held.append(k)
        del held[:-SLOTS]
    return out


def test_the_key_model_says_every_reuse_is_a_rebuild():
    keys = [k for _, k in walk_2d() if k is not None]
    assert len(set(keys)) == 26
    miss = lru_misses(keys)
    last_use = {k: j for j, k in enumerate(keys[:-11])}
    for j, k in enumerate(keys[-11:], start=len(keys) - 11):
        if keys[j - 1] != k:                                        # (m = 10, 9 and m = 8, 7 share a key: the second of a pair is a hit)
            assert miss[j] and len(set(keys[last_use[k] + 1:j]) - {k}) >= 17, k
    keys3 = [k for _, k in walk_3d() if k is not None]
    assert len(set(keys3)) == 18
    miss3 = lru_misses(keys3)
    assert all(miss3[j] or keys3[j - 1] == keys3[j] for j in range(len(keys3)))          # every first use of a pass rebuilds


# ---- data -----------------------------------------------------------------------------------------------------------------
def _matcher(dim, **kw):
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D
    kw.setdefault("cell_size", HL.CELL[dim])
    return (NdtMatcher2D if dim == 2 else NdtMatcher3D)(**kw)


def _cols(pts):
    return [np.ascontiguousarray(pts[:, a]) for a in range(pts.shape[1])]


def _dev(pts):
    import torch
    return tuple(torch.from_numpy(c).cuda() for c in _cols(pts))


_scenes = {}


def scene(dim):
    """A 20 000-point room, 40 scans of 5 000 points seen from poses near its centre, and a start pose for each."""
    if dim not in _scenes:
        rng = np.random.default_rng(77 + dim)
        world = HL._cloud(rng, dim, 20000, np.zeros(dim), 40.0, with_inf=False)
        fin = world[np.isfinite(world).all(axis=1)]
        scans, inits = [], []
        for _ in range(40):
            true = HL._small_pose(rng, dim, 0.5, 0.05)
            pick = fin[rng.integers(0, len(fin), 5000)]
            scans.append((HL._sensor_frame(dim, pick, true) + rng.normal(0, 0.01, (5000, dim))).astype(np.float32))
            inits.append(true + HL._small_pose(rng, dim, 0.08, 0.01))
        _scenes[dim] = dict(world=world, scans=scans, inits=np.stack(inits))
    return _scenes[dim]


def _flat(r):
    if isinstance(r, (list, tuple)):
        return [_flat(v) for v in r]
    if hasattr(r, "pose"):
        return [np.asarray(r.pose, np.float64), r.H, r.g, np.float64(r.score), np.int64(r.iterations), np.int64(r.n_hit), np.int64(r.status)]
    return np.asarray(r)


def _assert_same(got, want, where):
    got, want = _flat(got), _flat(want)

    def walk(u, v, at):
        if isinstance(v, list):
            assert len(u) == len(v), at
            for j, (a, b) in enumerate(zip(u, v)):
                walk(a, b, f"{at}[{j}]")
        else:
            assert u.dtype == v.dtype and u.shape == v.shape, at
            np.testing.assert_array_equal(np.ascontiguousarray(u).reshape(-1).view(np.uint8),
                                          np.ascontiguousarray(v).reshape(-1).view(np.uint8), err_msg=at)
    walk(got, want, where)


def _point_call(h, call, sc, dev):
    kind, m = call
    if kind == "multi_start":
        return h.align_multi_start(*dev[0], sc["inits"][:m])
    if kind == "multi_scan":
        return h.align_multi_scan(dev[:m], sc["inits"][:m])
    if kind == "align":
        return h.align(*dev[1], tuple(sc["inits"][1]))
    if kind == "evaluate":
        return h.evaluate(*dev[2], tuple(sc["inits"][2]))
    if kind == "align_trace":
        return h.align_trace(*_cols(sc["scans"][3]), tuple(sc["inits"][3]))
    raise KeyError(kind)


def _walk(dim, calls, **params):
    sc = scene(dim)
    dev = [_dev(s) for s in sc["scans"]]
    with _matcher(dim, **params) as h:
        h.set_target(*_cols(sc["world"]))
        blob = h.save_map()
        nb = 1
        for j, (call, key) in enumerate(calls):
            if call[0] == "neighbourhood":
                nb = call[1]
                h.set_neighbourhood(nb)
                continue
            got = _point_call(h, call, sc, dev)
            with _matcher(dim, **params) as fresh:
                fresh.load_map(blob)
                if nb != 1:
                    fresh.set_neighbourhood(nb)
                want = _point_call(fresh, call, sc, dev)
            _assert_same(got, want, f"call {j}: {call}, key {key}")
            if call[0].startswith("multi"):
                assert all(r.iterations > 0 for r in got), call      # the chains did run


def test_multi_start_shapes_2d(gpu_lib):
    _walk(2, walk_2d(), fixed_iterations=3)


def test_multi_start_shapes_3d(gpu_lib):
    _walk(3, walk_3d(), fixed_iterations=3)


# ---- map-to-map -------------------------------------------------------------------------------------------------------------
def _uniform(rng, dim, cells, per_cell):
    """A uniform cloud over about `cells` cells of a square (a 3 m slab in 3D) round the origin."""
    c = HL.CELL[dim]
    side = c * np.sqrt(cells / (1 if dim == 2 else 3))
    n = int(cells * per_cell)
    cols = [rng.uniform(-side / 2, side / 2, n), rng.uniform(-side / 2, side / 2, n)]
    if dim == 3:
        cols.append(rng.uniform(0.0, 3.0, n))
    return np.stack(cols, axis=1).astype(np.float32)


@pytest.mark.parametrize("dim", [2, 3])
def test_map_to_map_shapes(gpu_lib, dim):
    rng = np.random.default_rng(5 + dim)
    per_cell = 8 if dim == 2 else 12
    params = dict(fixed_iterations=3)
    sources = [_matcher(dim) for _ in range(20)]
    try:
        for j, s in enumerate(sources):
            s.set_target(*_cols(_uniform(rng, dim, 256 * (j + 1) - 128, per_cell)))
        blocks = [-(-len(s.components()[0]) // 256) for s in sources]
        assert len(set(blocks)) >= 17 and max(blocks) <= 256, blocks
        inits = np.stack([HL._small_pose(rng, dim, 0.1, 0.01) for _ in range(20)])
        with _matcher(dim, **params) as t:
            t.set_target(*_cols(_uniform(rng, dim, 256 * 20, per_cell)))
            blob = t.save_map()

            def fresh():
                f = _matcher(dim, **params)
                f.load_map(blob)
                return f

            for rnd in range(2):
                for j, s in enumerate(sources):
                    got = t.align_map(s, tuple(inits[j]))
                    with fresh() as f:
                        want = f.align_map(s, tuple(inits[j]))
                    _assert_same(got, want, f"round {rnd}, source {j}, blocks {blocks[j]}")
                    assert got.iterations > 0 and got.n_hit > 0
                    if j % 5 == 4:
                        m = (2, 5, 9, 17)[j // 5]
                        srcs = [sources[(j + 3 * k) % 20] for k in range(m)]
                        poses = np.stack([inits[(j + k) % 20] for k in range(m)])
                        got = t.align_map_multi(srcs, poses)
                        with fresh() as f:
                            want = f.align_map_multi(srcs, poses)
                        _assert_same(got, want, f"round {rnd}, align_map_multi of {m}")
    finally:
        for s in sources:
            s.close()


# ---- eviction while chains are queued ---------------------------------------------------------------------------------------
def _fill(h, sc, dev):
    """The 18 fused multi keys (2D) / 16 keys (3D: seven multi shapes, and evaluate, under both neighbourhoods): more than
    enough to push every single-chain graph out of the sixteen slots."""
    if len(dev[0]) == 2:
        for m in range(1, 12):
            h.align_multi_start(*dev[0], sc["inits"][:m])
            h.align_multi_scan(dev[:m], sc["inits"][:m])
    else:
        back = h.neighbourhood
        for nb in (1, 7):
            h.set_neighbourhood(nb)
            for m in (1, 2, 3, 5, 9, 17, 33):
                h.align_multi_start(*dev[0], sc["inits"][:m])
            h.evaluate(*dev[2], tuple(sc["inits"][2]))
        h.set_neighbourhood(back)


def _async_runs(dim, h, fresh, sc, dev, what):
    import torch
    torch.cuda.synchronize()                                        # the scans are complete: the calls go back to back
    first = 4
    for run in (1, 2, 3, 4):
        _fill(h, sc, dev)
        for q in range(first, first + run):
            h.align_async(*dev[q], tuple(sc["inits"][q]), producer_complete=True)
        got = h.finish()
        want = fresh.align(*dev[first + run - 1], tuple(sc["inits"][first + run - 1]))
        _assert_same(got, want, f"{what}: run of {run}")
        assert got.iterations > 0
        first += run


def test_eviction_while_lanes_are_busy_2d(gpu_lib):
    sc = scene(2)
    dev = [_dev(s) for s in sc["scans"]]
    with _matcher(2, fixed_iterations=30, tuning={"async_chains": 4}) as h, _matcher(2, fixed_iterations=30) as fresh:
        h.set_target(*_cols(sc["world"]))
        fresh.load_map(h.save_map())
        _async_runs(2, h, fresh, sc, dev, "lane_fork 0")
        h.set_tuning("lane_fork", 1)
        _async_runs(2, h, fresh, sc, dev, "lane_fork 1")


def test_eviction_in_front_of_async_runs_3d(gpu_lib):
    sc = scene(3)
    dev = [_dev(s) for s in sc["scans"]]
    with _matcher(3, fixed_iterations=30) as h, _matcher(3, fixed_iterations=30) as fresh:
        h.set_target(*_cols(sc["world"]))
        fresh.load_map(h.save_map())
        for nb in (1, 7):
            h.set_neighbourhood(nb)
            fresh.set_neighbourhood(nb)
            _async_runs(3, h, fresh, sc, dev, f"neighbourhood {nb}")
