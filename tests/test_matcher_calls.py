"""gtsam_ndt_amd/matcher.py against a recording stand-in for the library: which C functions every public method of the
matcher, batch, multi-device and pyramid classes calls, in which order, with how many and which kinds of arguments - once
for ndt2d_* and once for ndt3d_*, from one table.  Needs neither a device nor the built library."""
import ctypes as C

import numpy as np
import pytest
import torch

from gtsam_ndt_amd import _lib as L
from gtsam_ndt_amd import matcher as M

N, PAIRS = 5, 2


class StubLib:
    """Every name of L.SIGNATURES as a callable that checks its arguments against the signature, records the call and
    returns 0 (or `returns[name]`); the create functions hand out handles 0x100, 0x200, ..."""

    def __init__(self):
        self.calls, self.returns, self._handles = [], {}, 0

    def __getattr__(self, name):
        if name not in L.SIGNATURES:
            raise AttributeError(name)
        argtypes = L.SIGNATURES[name][1]

        def fn(*args):
            assert len(args) == len(argtypes), f"{name} takes {len(argtypes)} arguments, got {len(args)}"
            for a, t in zip(args, argtypes):
                t.from_param(a)
            self.calls.append((name, args))
            if name in ("ndt_status_string", "ndt_last_error"):
                return b"stub"
            if "_create" in name and self.returns.get(name, 0) >= 0:
                self._handles += 0x100
                args[-1]._obj.value = self._handles
            if name.endswith("_get_components") and args[1] is None:
                args[-1]._obj.value = 4                       # four valid cells: the method comes back for them
            return self.returns.get(name, 0)
        setattr(self, name, fn)
        return fn

    def names(self):
        return [name for name, _ in self.calls]


class FakeTensor:
    """What matcher.py asks of a device array."""
    is_cuda, device = True, "cuda:0"

    def __init__(self, ptr, n, dtype=torch.float32):
        self._ptr, self._n, self.dtype = ptr, n, dtype

    def numel(self):
        return self._n

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return self._ptr


class FakeStream:
    cuda_stream = 0x5000

    def __init__(self):
        self.waited = []

    def wait_stream(self, other):
        self.waited.append(other)


class Env:
    """The objects the cases run on, for one dimension (d = 2 or 3)."""

    def __init__(self, d):
        self.d, self.npose = d, 3 * (d - 1)
        suffix = f"{d}D"
        self.Matcher, self.Batch, self.Multi = (getattr(M, k + suffix) for k in ("NdtMatcher", "NdtBatch", "NdtMulti"))
        self.Pyramid, self.MapPyramid = getattr(M, "NdtPyramid" + suffix), getattr(M, "NdtMapPyramid" + suffix)
        self.Result = getattr(L, "Result" + suffix)
        self.host = tuple(np.arange(N, dtype=np.float32) + a for a in range(d))
        self.dev = tuple(FakeTensor(0x1000 * (a + 1), N) for a in range(d))
        self.pose = tuple(0.1 * (a + 1) for a in range(self.npose))
        self.window = (self.pose, (1.0, 1.0, 0.2), (0.5, 0.5, 0.1))
        self.lo_hi = ((-1.0, -2.0, 3.0, 4.0) if d == 2 else ((-1.0, -2.0, -3.0), (1.0, 2.0, 3.0)))
        # a batch of PAIRS pairs, on the host and on the device
        self.clouds = [self.host] * PAIRS
        self.inits = [self.pose] * PAIRS
        cat = lambda base: tuple(FakeTensor(base + 0x1000 * a, N * PAIRS) for a in range(d))
        self.t, self.s = cat(0x10000), cat(0x20000)
        self.toff, self.soff = (FakeTensor(p, PAIRS + 1, torch.int64) for p in (0x30000, 0x31000))
        self.init = FakeTensor(0x32000, PAIRS * self.npose, torch.float64)
        self.out = FakeTensor(0x33000, PAIRS * self.Result.__sizeof__(self.Result) // 8, torch.float64)

    def objects(self):
        self.m, self.src, self.coarse = self.Matcher(), self.Matcher(), self.Matcher()
        self.batch, self.multi = self.Batch(), self.Multi()
        self.pyr, self.mpyr, self.mpyr_src = self.Pyramid(), self.MapPyramid(self.m), self.MapPyramid(self.src)

    def batch_align_dev(self, **kw):
        if self.d == 2:
            return self.batch.align_dev(*self.t, self.toff, *self.s, self.soff, self.init, out=self.out, **kw)
        return self.batch.align_dev(self.t, self.toff, self.s, self.soff, self.init, out=self.out, **kw)

    def shard(self):
        if self.d == 2:
            return dict(tx=self.t[0], ty=self.t[1], toff=self.toff, sx=self.s[0], sy=self.s[1], soff=self.soff,
                        init=self.init)
        return dict(t=self.t, toff=self.toff, s=self.s, soff=self.soff, init=self.init)


LEVEL = ["{p}_default_params", "{p}_create"]
MAP_LEVEL = LEVEL + ["{p}_coarsen_map", "{p}_get_grid_info"]

# id: (the call, the C functions it makes, the one that fails in the error test, the NdtError's where if it is not that
# function's name)
CASES = {
    "create": (lambda e: e.Matcher(0, tuning={"launch_graphs": 0}), LEVEL + ["{p}_set_tuning"], "{p}_create", None),
    "set_tuning": (lambda e: e.m.set_tuning("fused_begin", 1), ["{p}_set_tuning"], "{p}_set_tuning", None),
    "set_target host": (lambda e: e.m.set_target(*e.host), ["{p}_set_target", "{p}_get_grid_info"], "{p}_set_target", None),
    "set_target dev": (lambda e: e.m.set_target(*e.dev), ["{p}_set_target_dev", "{p}_get_grid_info"], "{p}_set_target_dev",
                       {2: "ndt2d_set_target", 3: "ndt3d_set_target_dev"}),
    "reserve_target": (lambda e: e.m.reserve_target(*e.lo_hi), ["{p}_reserve_target", "{p}_get_grid_info"],
                       "{p}_reserve_target", None),
    "add host": (lambda e: e.m.add_target_points(*e.host), ["{p}_add_target_points"], "{p}_add_target_points", None),
    "add dev": (lambda e: e.m.add_target_points(*e.dev, pose=e.pose), ["{p}_add_target_points_dev"],
                "{p}_add_target_points_dev", None),
    "add dev no pose": (lambda e: e.m.add_target_points(*e.dev), ["{p}_add_target_points_dev"], None, None),
    "remove host": (lambda e: e.m.remove_target_points(*e.host), ["{p}_remove_target_points"], "{p}_remove_target_points", None),
    "remove dev": (lambda e: e.m.remove_target_points(*e.dev, pose=e.pose), ["{p}_remove_target_points_dev"],
                   "{p}_remove_target_points_dev", None),
    "grid_info": (lambda e: e.m.grid_info(), ["{p}_get_grid_info"], "{p}_get_grid_info", None),
    "grid": (lambda e: e.m.grid(), ["{p}_get_grid_info", "{p}_get_grid"], "{p}_get_grid", None),
    "save_map": (lambda e: e.m.save_map(), ["{p}_map_size", "{p}_save_map"], "{p}_save_map", None),
    "load_map": (lambda e: e.m.load_map(np.zeros(128, np.uint8)), ["{p}_load_map"], "{p}_load_map", None),
    "load_map bytes": (lambda e: e.m.load_map(bytes(128)), ["{p}_load_map"], None, None),
    "coarsen_into": (lambda e: e.m.coarsen_into(e.coarse), ["{p}_coarsen_map", "{p}_get_grid_info"], "{p}_coarsen_map", None),
    "evaluate host": (lambda e: e.m.evaluate(*e.host, e.pose), ["{p}_evaluate"], "{p}_evaluate", None),
    "evaluate dev": (lambda e: e.m.evaluate(*e.dev, e.pose), ["{p}_wait_stream", "{p}_evaluate_dev"], "{p}_evaluate_dev", None),
    "wait_stream": (lambda e: e.m.wait_stream(), ["{p}_wait_stream"], "{p}_wait_stream", None),
    "wait_stream given": (lambda e: e.m.wait_stream(0x6000), ["{p}_wait_stream"], None, None),
    "align host": (lambda e: e.m.align(*e.host, e.pose), ["{p}_align"], "{p}_align", None),
    "align host default": (lambda e: e.m.align(*e.host), ["{p}_align"], None, None),
    "align dev": (lambda e: e.m.align(*e.dev, init_pose=e.pose), ["{p}_wait_stream", "{p}_align_dev"], "{p}_align_dev", "{p}_align"),
    "align dev wait": (lambda e: e.m.align(*e.dev), ["{p}_wait_stream", "{p}_align_dev"], "{p}_wait_stream", None),
    "align_map": (lambda e: e.m.align_map(e.src, e.pose), ["{p}_align_map"], "{p}_align_map", None),
    "align_map default": (lambda e: e.m.align_map(e.src), ["{p}_align_map"], None, None),
    "align_map_multi one": (lambda e: e.m.align_map_multi(e.src, [e.pose] * 3), ["{p}_align_map_multi"], "{p}_align_map_multi", None),
    "align_map_multi list": (lambda e: e.m.align_map_multi([e.src, e.m], [e.pose] * 2), ["{p}_align_map_multi"], None, None),
    "evaluate_map": (lambda e: e.m.evaluate_map(e.src, e.pose), ["{p}_evaluate_map"], "{p}_evaluate_map", None),
    "components": (lambda e: e.m.components(), ["{p}_get_components"] * 2, "{p}_get_components", None),
    "align_trace": (lambda e: e.m.align_trace(*e.host, init_pose=e.pose, capacity=8), ["{p}_align_trace"], "{p}_align_trace", None),
    "align_multi_start": (lambda e: e.m.align_multi_start(*e.dev, [e.pose] * 3), ["{p}_wait_stream", "{p}_align_multi_start_dev"],
                          "{p}_align_multi_start_dev", None),
    "align_multi_scan": (lambda e: e.m.align_multi_scan([e.dev] * 2, [e.pose] * 2), ["{p}_wait_stream", "{p}_align_multi_scan_dev"],
                         "{p}_align_multi_scan_dev", None),
    "search host": (lambda e: e.m.search(*e.host, *e.window, k=4, min_sep=(0.3, 0.2)), ["{p}_search"], "{p}_search", None),
    "search dev": (lambda e: e.m.search(*e.dev, *e.window), ["{p}_wait_stream", "{p}_search_dev"], "{p}_search_dev", "{p}_search"),
    "search_align": (lambda e: e.m.search_align(*e.dev, *e.window, k=4), ["{p}_wait_stream", "{p}_search_align_dev"],
                     "{p}_search_align_dev", None),
    "search_map": (lambda e: e.m.search_map(e.src, *e.window, k=4), ["{p}_search_map"], "{p}_search_map", None),
    "search_align_map": (lambda e: e.m.search_align_map(e.src, *e.window, min_sep=(0.3, 0.2)), ["{p}_search_align_map"],
                         "{p}_search_align_map", None),
    "align_async": (lambda e: e.m.align_async(*e.dev, init_pose=e.pose), ["{p}_wait_stream", "{p}_align_dev_async"],
                    "{p}_align_dev_async", None),
    "align_async complete": (lambda e: e.m.align_async(*e.dev, producer_complete=True), ["{p}_align_dev_async"], None, None),
    "finish": (lambda e: e.m.finish(), ["{p}_align_finish"], "{p}_align_finish", None),
    "stream": (lambda e: e.m.stream, ["{p}_stream"], None, None),
    "with": (lambda e: e.src.__exit__(None, None, None), ["{p}_destroy"], None, None),
    # ---- batch
    "batch create": (lambda e: e.Batch(1), ["{p}_default_params", "{p}_batch_create"], "{p}_batch_create", None),
    "batch create levels": (lambda e: e.Batch(levels=[M.default_params()] * 2, global_workgroups=8),
                            ["ndt2d_default_params", "{p}_default_params", "{p}_batch_create_pyramid", "{p}_batch_set_tuning"],
                            "{p}_batch_create_pyramid", None),
    "batch set_tuning": (lambda e: e.batch.set_tuning("batch_global_workgroups", 4), ["{p}_batch_set_tuning"],
                         "{p}_batch_set_tuning", None),
    "batch stream": (lambda e: e.batch.stream, ["{p}_batch_stream"], None, None),
    "batch align": (lambda e: e.batch.align(e.clouds, e.clouds, e.inits), ["{p}_batch_align"], "{p}_batch_align", None),
    "batch align_dev stream": (lambda e: e.batch_align_dev(stream=0x7000), ["{p}_batch_align_dev"], "{p}_batch_align_dev", None),
    "batch align_dev": (lambda e: e.batch_align_dev(), ["{p}_batch_wait_stream", "{p}_batch_align_dev", "{p}_batch_stream"],
                        "{p}_batch_wait_stream", None),
    "batch decode": (lambda e: e.Batch.decode(torch.zeros((PAIRS, C.sizeof(e.Result) // 8), dtype=torch.float64)), [], None, None),
    "batch close": (lambda e: e.batch.close(), ["{p}_batch_destroy"], None, None),
    # ---- multi-device
    "multi create": (lambda e: e.Multi(), ["{p}_default_params", "{p}_multi_create"], "{p}_multi_create", None),
    "multi create levels": (lambda e: e.Multi(devices=[0, 1], levels=M.pyramid_params()),
                            ["ndt2d_default_params", "ndt2d_default_pyramid", "{p}_default_params", "{p}_multi_create_pyramid"],
                            "{p}_multi_create_pyramid", None),
    "multi device_count": (lambda e: e.multi.device_count, ["{p}_multi_device_count"], None, None),
    "multi align": (lambda e: e.multi.align(e.clouds, e.clouds, e.inits), ["{p}_multi_align"], "{p}_multi_align", None),
    "multi align_dev": (lambda e: e.multi.align_dev([e.shard(), None]), ["{p}_multi_device_count", "{p}_multi_align_dev"],
                        "{p}_multi_align_dev", None),
    "multi close": (lambda e: e.multi.close(), ["{p}_multi_destroy"], None, None),
    # ---- pyramids
    "pyramid create": (lambda e: e.Pyramid(), ["{p}_default_params"] + LEVEL * 3, "{p}_create", None),
    "pyramid set_target": (lambda e: e.pyr.set_target(*e.host), ["{p}_set_target", "{p}_get_grid_info"] * 3, "{p}_set_target", None),
    "pyramid align": (lambda e: e.pyr.align(*e.host, e.pose), ["{p}_align"] * 3, "{p}_align", None),
    "pyramid align dev": (lambda e: e.pyr.align(*e.dev), ["{p}_wait_stream", "{p}_align_dev"] * 3, None, None),
    "pyramid close": (lambda e: e.pyr.close(), ["{p}_destroy"] * 3, None, None),
    "map pyramid create": (lambda e: e.MapPyramid(e.m), MAP_LEVEL * 2, "{p}_coarsen_map", None),
    "map pyramid from_blob": (lambda e: e.MapPyramid.from_blob(np.zeros(256, np.uint8)).close(),
                              LEVEL + ["{p}_load_map"] + MAP_LEVEL * 2 + ["{p}_destroy"] * 3, "{p}_load_map", None),
    "map pyramid align_map": (lambda e: e.mpyr.align_map(e.mpyr_src, e.pose), ["{p}_align_map"] * 3, "{p}_align_map", None),
    "map pyramid align_map default": (lambda e: e.mpyr.align_map(e.mpyr_src), ["{p}_align_map"] * 3, None, None),
    "map pyramid close": (lambda e: e.mpyr.close(), ["{p}_destroy"] * 2, None, None),
}


@pytest.fixture
def stub(monkeypatch):
    lib = StubLib()
    lib.returns.update(ndt2d_multi_device_count=2, ndt3d_multi_device_count=2)
    lib.torch_stream, lib.synchronized = FakeStream(), []
    monkeypatch.setattr(L, "load", lambda: lib)
    monkeypatch.setattr(M, "_torch_stream", lambda: lib.torch_stream)
    monkeypatch.setattr(torch.cuda, "ExternalStream", lambda ptr: ("external", ptr))
    monkeypatch.setattr(torch.cuda, "synchronize", lib.synchronized.append)
    return lib


def address(a):
    """A pointer argument's address, handed over as an int or as a c_void_p."""
    return getattr(a, "value", a)


def main_call(calls):
    """The arguments of the call a case is about: not the stream ordering before it or the grid_info after it."""
    return [args for name, args in calls if not name.endswith(("_wait_stream", "_get_grid_info"))][0]


def run_case(stub, d, case):
    """The calls of one case, on fresh objects."""
    env = Env(d)
    env.objects()
    del stub.calls[:]
    made = CASES[case][0](env)          # held until the calls are copied: freeing a handle is a call too
    calls = list(stub.calls)
    del made
    return calls


@pytest.mark.parametrize("d", [2, 3])
def test_every_method_makes_its_calls_in_order(stub, d):
    for case, (_, expected, _, _) in CASES.items():
        names = [name for name, _ in run_case(stub, d, case)]
        assert names == [n.format(p=f"ndt{d}d") for n in expected], case


@pytest.mark.parametrize("d", [2, 3])
def test_a_negative_status_raises_with_the_where_of_the_call(stub, d):
    p = f"ndt{d}d"
    for case, (call, _, failing, where) in CASES.items():
        if failing is None:
            continue
        failing = failing.format(p=p)
        where = where[d] if isinstance(where, dict) else (where or failing).format(p=p)
        env = Env(d)
        env.objects()
        stub.returns[failing] = -1
        with pytest.raises(L.NdtError, match=f"^{where}: stub") as err:
            call(env)
        assert err.value.code == -1, case
        del stub.returns[failing]


@pytest.mark.parametrize("d", [2, 3])
def test_pose_length_and_struct_types(stub, d):
    env = Env(d)
    pose_t, result_t, eval_t = C.c_double * env.npose, env.Result, getattr(L, f"Eval{d}D")
    byref_of = lambda a: type(a._obj)
    for case, pose_at, out_at, out_t in (("align host", -2, -1, result_t), ("align dev", -2, -1, result_t),
                                         ("evaluate host", -2, -1, eval_t), ("evaluate dev", -2, -1, eval_t),
                                         ("align_map", -2, -1, result_t), ("align_map default", -2, -1, result_t),
                                         ("evaluate_map", -2, -1, eval_t), ("align_async", -1, None, None),
                                         ("add dev", -3, None, None), ("remove dev", -3, None, None),
                                         ("align_trace", 2 + d, None, None), ("finish", None, -1, result_t)):
        args = run_case(stub, d, case)[-1][1]
        if pose_at is not None:
            assert type(args[pose_at]) is pose_t, case
            want = (0.0,) * env.npose if case == "align_map default" else env.pose
            assert tuple(args[pose_at]) == want, case
        if out_at is not None:
            assert byref_of(args[out_at]) is out_t, case
    assert run_case(stub, d, "add dev no pose")[-1][1][-3] is None
    assert byref_of(run_case(stub, d, "grid_info")[-1][1][-1]) is getattr(L, f"GridInfo{d}D")
    window = byref_of(run_case(stub, d, "search host")[-1][1][-4])
    assert window is getattr(L, f"SearchWindow{d}D") and len(window().center) == env.npose
    # the coordinate pointers: one per axis, then the one length they share
    for case in ("set_target host", "align host", "evaluate host", "search host", "align_trace"):
        args = main_call(run_case(stub, d, case))
        assert len(set(args[1:1 + d])) == d and args[1 + d] == N, case
    for case in ("set_target dev", "align dev", "align_async", "search dev", "align_multi_start"):
        args = main_call(run_case(stub, d, case))
        assert [address(a) for a in args[1:1 + d]] == [t.data_ptr() for t in env.dev] and args[1 + d] == N, case
    # the batch layouts: clouds, offsets, clouds, offsets, initial poses, pair count, rows, stream
    args = run_case(stub, d, "batch align_dev stream")[-1][1]
    want = [*env.t, env.toff, *env.s, env.soff, env.init]
    assert [address(a) for a in args[1:len(want) + 1]] == [t.data_ptr() for t in want]
    assert args[-3] == PAIRS and address(args[-2]) == env.out.data_ptr() and address(args[-1]) == 0x7000
    calls = run_case(stub, d, "multi align_dev")
    assert [list(column) for column in calls[-1][1][1:len(want) + 1]] == [[t.data_ptr(), None] for t in want]
    assert list(calls[-1][1][len(want) + 1]) == [PAIRS, 0]


@pytest.mark.parametrize("d", [2, 3])
def test_streams_are_ordered_around_the_device_calls(stub, d):
    args = run_case(stub, d, "wait_stream")[-1][1]
    assert args[1].value == FakeStream.cuda_stream
    assert run_case(stub, d, "wait_stream given")[-1][1][1].value == 0x6000
    for case in ("set_target dev", "add dev", "remove dev"):            # these take torch's stream themselves
        assert run_case(stub, d, case)[0][1][-1].value == FakeStream.cuda_stream, case
    stub.returns[f"ndt{d}d_batch_stream"] = 0x8000
    calls = run_case(stub, d, "batch align_dev")                         # wait in, run on the context's stream, wait out
    assert calls[0][1][1].value == FakeStream.cuda_stream and not calls[1][1][-1].value
    assert stub.torch_stream.waited == [("external", 0x8000)]
    stub.torch_stream.waited.clear()
    run_case(stub, d, "batch align_dev stream")                          # the caller's stream: no ordering either way
    assert stub.torch_stream.waited == []
    del stub.synchronized[:]
    run_case(stub, d, "multi align_dev")
    assert stub.synchronized == ["cuda:0"]                              # once per shard that holds pairs


@pytest.mark.parametrize("d", [2, 3])
def test_close_destroys_the_handle_once(stub, d):
    env = Env(d)
    for make, destroy in ((env.Matcher, "_destroy"), (env.Batch, "_batch_destroy"), (env.Multi, "_multi_destroy")):
        obj = make()
        handle = obj._h.value
        del stub.calls[:]
        obj.close()
        obj.close()
        del obj
        assert [(n, a[0].value) for n, a in stub.calls] == [(f"ndt{d}d{destroy}", handle)]
    with env.Matcher() as m:
        del stub.calls[:]
    assert stub.names() == [f"ndt{d}d_destroy"] and m._h is None


def test_what_only_the_2d_classes_have(stub):
    params = M.default_params(cell_size=2.0)
    for make in (lambda **kw: M.NdtMatcher2D(0, **kw), lambda **kw: M.NdtBatch2D(0, **kw), lambda **kw: M.NdtMulti2D(None, **kw)):
        del stub.calls[:]
        obj = make(params=params, min_points=7)
        assert obj.params is params and params.min_points == 7
        assert "ndt2d_default_params" not in stub.names()
    del stub.calls[:]
    batch = M.NdtBatch2D(small_variant=False, global_workgroups=16)
    assert stub.names() == ["ndt2d_default_params", "ndt2d_batch_create", "ndt2d_batch_set_tuning", "ndt2d_batch_set_tuning"]
    assert [a[1:] for _, a in stub.calls[2:]] == [(L.TUNING["batch_small_variant"], 0), (L.TUNING["batch_global_workgroups"], 16)]
    stub.returns["ndt2d_batch_last_large_count"] = 3
    assert batch.last_large_count == 3
    assert M.NdtMulti2D().last_shard_stride == 0 and M.NdtMulti3D().last_shard_stride == 0
    assert M.NdtMatcher3D()._keep is None


@pytest.mark.parametrize("d", [2, 3])
def test_host_clouds_must_be_1d_and_equally_long(stub, d):
    env = Env(d)
    env.objects()
    short = env.host[:-1] + (env.host[-1][:-1],)
    flat = tuple(a.reshape(1, N) for a in env.host)
    del stub.calls[:]
    for bad in (short, flat):
        with pytest.raises(ValueError, match="must be 1-D arrays of equal length"):
            M._host_coords(bad)
        for call in (lambda: env.m.set_target(*bad), lambda: env.m.add_target_points(*bad),
                     lambda: env.m.remove_target_points(*bad), lambda: env.m.evaluate(*bad, env.pose),
                     lambda: env.m.align(*bad), lambda: env.m.align_trace(*bad), lambda: env.m.search(*bad, *env.window),
                     lambda: env.pyr.set_target(*bad), lambda: env.batch.align([bad], [env.host], [env.pose]),
                     lambda: env.multi.align([env.host], [bad], [env.pose])):
            with pytest.raises(ValueError, match="must be 1-D arrays of equal length"):
                call()
    assert stub.calls == []                                              # refused before anything reaches the library
    assert [a.dtype for a in M._host_coords([list(range(N))] * d)] == [np.float32] * d
