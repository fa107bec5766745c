"""The schedules of tests/handle_life.py, replayed on the model alone (no GPU): what tests/test_gpu_handle_life.py relies
on when it walks real handles through them.  These are conditions on the schedules, not measurements.

Seeds: 0 and 1 were tried for both dimensions (and 1000, 1001 for the overlap_grids = 4 run) and satisfy every condition
below; no seed was rejected."""
import collections
import time

import numpy as np
import pytest

import handle_life as HL

CASES = [(2, 0), (2, 1), (3, 0), (3, 1)]             # the (dim, seed) of tests/test_gpu_handle_life.py
_replays = {}
_seconds = {}


def replay(dim, seed):
    """[(step, prediction, blob of the step's handle afterwards or None, largest cell count)] - computed once, shared."""
    if (dim, seed) not in _replays:
        t0 = time.perf_counter()
        life = HL.Life(dim)
        out = []
        for step in HL.schedule(dim, seed):
            pred = life.apply(step)
            m = life.model[step[1]]
            out.append((step, pred, m.blob() if m.has_target else None, m.max_count(), m.n_valid() if m.has_target else None))
        _replays[(dim, seed)] = out
        _seconds[(dim, seed)] = time.perf_counter() - t0
    return _replays[(dim, seed)]


@pytest.mark.parametrize("dim,seed", CASES)
def test_every_kind_of_step_occurs_often_enough(dim, seed):
    rep = replay(dim, seed)
    went_well = collections.Counter(step[0] for step, pred, *_ in rep if pred["status"] == HL.NDT_OK)
    for op in HL.MUTATORS + HL.QUERIES:
        assert went_well[op] >= 2, (op, went_well[op])
    failed = collections.Counter((step[0], pred["status"]) for step, pred, *_ in rep if pred["kind"] == "mutator" and pred["status"] != HL.NDT_OK)
    assert failed[("remove", HL.NDT_ERR_INVALID_ARG)] >= 1 and failed[("merge", HL.NDT_ERR_CAPACITY)] >= 1
    for who in (0, 1):                                               # each handle is mutated, queried, and target and source of a map call
        assert sum(1 for step, pred, *_ in rep if step[1] == who and pred["kind"] == "mutator") >= 8
        assert sum(1 for step, pred, *_ in rep if step[1] == who and step[0] in HL.MAP_QUERIES and pred["status"] == HL.NDT_OK) >= 2
    sizes = [len(step[2]) for step, *_ in rep if step[0] in ("align", "align_host")]
    assert min(sizes) <= 4096 < max(sizes)                           # both sides of the short-scan limit
    runs = {len(step[2]) for step, *_ in rep if step[0] == "align_async"}
    assert runs and runs <= {1, 2, 3, 4}
    ms = [len(step[3]) for step, *_ in rep if step[0] in ("multi_start", "multi_scan")]
    assert min(ms) >= 1 and max(ms) <= 64
    if dim == 3:
        assert [step[2] for step, *_ in rep if step[0] == "set_neighbourhood"].count(7) >= 2
        assert [step[2] for step, *_ in rep if step[0] == "set_neighbourhood"][-1] == 1
    targets = [len(step[2]) for step, *_ in rep if step[0] == "set_target"]
    assert min(targets) == 300 and max(targets) == 20000
    assert any(np.isnan(step[2]).any() for step, *_ in rep if step[0] in ("set_target", "add"))
    assert any(np.isinf(step[2]).any() for step, *_ in rep if step[0] in ("add", "remove"))


@pytest.mark.parametrize("dim,seed", CASES)
def test_failures_are_the_planned_ones_and_queries_see_a_target(dim, seed):
    """The mutators that fail are removals of points that are not in the map (INVALID_ARG) and merges past 2^20 (CAPACITY);
    a query answers NO_TARGET exactly between such a failure on a handle it involves and that handle's next load."""
    rep = replay(dim, seed)
    down = [False, False]
    n_behind = 0
    for step, pred, *_ in rep:
        op, who = step[0], step[1]
        if pred["kind"] == "mutator":
            if pred["status"] != HL.NDT_OK:
                assert (op, pred["status"]) in (("remove", HL.NDT_ERR_INVALID_ARG), ("merge", HL.NDT_ERR_CAPACITY)), step[:2]
                assert not down[who]
                down[who] = True
            else:
                assert not down[who] or op == "load"                # the last good map comes back by load
                down[who] = False
        elif pred["kind"] == "query":
            involved = (who, 1 - who) if op in HL.MAP_QUERIES else (who,)
            want = HL.NDT_ERR_NO_TARGET if any(down[w] for w in involved) else HL.NDT_OK
            assert pred["status"] == want, step[:2]
            n_behind += want != HL.NDT_OK
    assert not any(down) and n_behind >= 4


@pytest.mark.parametrize("dim,seed", CASES)
def test_no_cell_passes_the_capacity(dim, seed):
    assert max(mx for *_, mx, _ in replay(dim, seed)) == HL.R.MAX_CELL_COUNT          # reached by the forged merges, never passed


@pytest.mark.parametrize("dim,seed", CASES)
def test_add_then_remove_gives_the_blob_back(dim, seed):
    rep = replay(dim, seed)
    pairs = 0
    for j, (step, pred, blob, *_) in enumerate(rep):
        if step[0] != "remove" or pred["status"] != HL.NDT_OK:
            continue
        for i in range(j - 1, -1, -1):
            s, p = rep[i][0], rep[i][1]
            if s[1] == step[1] and p["kind"] == "mutator":
                break
        assert s[0] == "add" and s[2] is step[2] and s[3] is step[3]     # the same cloud at the same pose
        assert pred["n_outside"] == p["n_outside"]
        before = next(rep[k][2] for k in range(i - 1, -1, -1) if rep[k][0][1] == step[1] and rep[k][1]["kind"] == "mutator")
        np.testing.assert_array_equal(blob, before)
        pairs += 1
    assert pairs >= 2


def test_merge_then_unmerge_gives_the_blob_back():
    for dim, seed in CASES:
        rep = replay(dim, seed)
        for j, (step, pred, blob, *_) in enumerate(rep):
            if step[0] == "unmerge":
                i = max(k for k in range(j) if rep[k][0][0] == "merge" and rep[k][0][2] is step[2])
                before = next(rep[k][2] for k in range(i - 1, -1, -1) if rep[k][0][1] == step[1] and rep[k][1]["kind"] == "mutator")
                np.testing.assert_array_equal(blob, before)


def test_n_valid_is_the_exact_records_count():
    """The model counts valid cells by integers alone; on the small targets of the schedules that is the count of
    cell_record_ref.exact_records (which needs an eigen-decomposition per cell and is too slow for every step)."""
    import cell_record_ref as CR
    checked = 0
    for dim, seed in CASES:
        for step, pred, blob, _, n_valid in replay(dim, seed):
            if step[0] == "set_target" and len(step[2]) == 300:
                assert n_valid == int(CR.exact_records(blob, HL.MIN_POINTS[dim], 1e-3)["valid"].sum())
                checked += 1
    assert checked >= 4


def test_the_short_schedule_keeps_a_rebuild_from_points_possible():
    for seed in (0, 1):
        steps = HL.short_schedule(seed)
        ops = [s[0] for s in steps]
        assert ops[0] == "reserve" and set(ops) <= {"reserve", "add", "remove"} | set(HL.POINT_QUERIES)
        assert ops.count("add") >= 3 and ops.count("remove") >= 2 and all(s[1] == 0 for s in steps)
        life = HL.Life(2)
        assert all(life.apply(s)["status"] == HL.NDT_OK for s in steps)


def test_the_replay_is_quick():
    for case in CASES:
        replay(*case)
    assert sum(_seconds.values()) < 20.0, _seconds                   # all seeds together: well under a minute
