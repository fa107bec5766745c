"""The staging and life-cycle code that the 2D and the 3D batch context share (csrc/ndt_batch_host.hpp), and the
multi-device context on top of it: a context that is used again with more and with fewer pairs, a multi-device context
with an empty shard, the tuning knobs and the 3D refusal of overlapping grids.  Results are compared as raw bytes:
the fixed-iteration path is deterministic (test_batch_fixed_iterations_and_determinism)."""
import ctypes as C

import numpy as np
import pytest

from gtsam_ndt_amd import synth, synth3d

pytestmark = pytest.mark.gpu

POSES3 = [(0.30, -0.20, 0.05, 0.01, -0.01, 0.03), (-0.25, 0.15, -0.04, -0.008, 0.012, -0.02), (0.10, 0.28, 0.02, 0.0, 0.015, 0.035)]


def _dim2():
    from gtsam_ndt_amd import matcher as M
    base = [synth.make_pair(4, pair_index=k, n_tgt=300, n_src=300) for k in range(3)]      # 300 points in a 50 m room:
    return dict(dim=2, pose=3, Batch=M.NdtBatch2D, Multi=M.NdtMulti2D, prefix="ndt2d", doubles=M.RESULT_DOUBLES, base=base,
                kw=dict(fixed_iterations=4, cell_size=4.0))                                  # 13 x 13 cells


def _dim3():
    from gtsam_ndt_amd import matcher as M
    base = [synth3d.make_pair3d(n_elev=6, n_azim=256, pose=p) for p in POSES3]             # 1536 points in a 40 m room:
    return dict(dim=3, pose=6, Batch=M.NdtBatch3D, Multi=M.NdtMulti3D, prefix="ndt3d", doubles=M.RESULT3_DOUBLES, base=base,
                kw=dict(fixed_iterations=4, cell_size=8.0))                                  # 5 x 5 x 1 voxels


@pytest.fixture(scope="module", params=["2d", "3d"])
def dims(request, gpu_lib):
    return _dim2() if request.param == "2d" else _dim3()


def _pairs(d, n, first=0):
    """n ragged pairs cut from the few generated ones: pair k drops the last 16 (k % 7) points of both clouds"""
    T, S, I = [], [], []
    for k in range(first, first + n):
        p = d["base"][k % len(d["base"])]
        keep = len(p["tx"]) - 16 * (k % 7)
        T.append(tuple(p["t" + a][:keep] for a in "xyz"[:d["dim"]]))
        S.append(tuple(p["s" + a][:keep] for a in "xyz"[:d["dim"]]))
        I.append(p["init"])
    return T, S, I


def _raw_align(d, ctx, what, T, S, I):
    """ndt?d_<what>_align on host pointers: the result rows as they come back, byte for byte"""
    from gtsam_ndt_amd import _lib as L
    n = len(T)
    toff = np.zeros(n + 1, dtype=np.uint64)
    soff = np.zeros(n + 1, dtype=np.uint64)
    toff[1:] = np.cumsum([len(t[0]) for t in T])
    soff[1:] = np.cumsum([len(s[0]) for s in S])
    t = [np.concatenate([np.ascontiguousarray(c[a], dtype=np.float32) for c in T]) for a in range(d["dim"])]
    s = [np.concatenate([np.ascontiguousarray(c[a], dtype=np.float32) for c in S]) for a in range(d["dim"])]
    init = np.ascontiguousarray(I, dtype=np.float64).reshape(n, d["pose"])
    out = np.zeros(n * d["doubles"], dtype=np.float64)
    name = f"{d['prefix']}_{what}_align"
    L.check(getattr(ctx._lib, name)(ctx._h, *[x.ctypes.data for x in t], toff.ctypes.data, *[x.ctypes.data for x in s],
                                    soff.ctypes.data, init.ctypes.data, n, out.ctypes.data), name)
    return out.tobytes()


def _status(d, raw):
    """the status word of every row (the last int32 but one of ndt2d_result / ndt3d_result)"""
    return np.frombuffer(raw, dtype=np.int32).reshape(-1, 2 * d["doubles"])[:, -2]


def test_reused_context_regrows_and_keeps_oversized_buffers(dims):
    """1 pair, then 70, then 2 on one context: with the slack rule k + k / 4 + 64 the second call is past every
    capacity the first left (66 offsets and rows, the points of one pair), the third finds every buffer oversized."""
    d = dims
    calls = [_pairs(d, 1), _pairs(d, 70, first=1), _pairs(d, 2, first=5)]
    with d["Batch"](**d["kw"]) as b:
        reused = [_raw_align(d, b, "batch", *c) for c in calls]
    for c, got in zip(calls, reused):
        with d["Batch"](**d["kw"]) as fresh:
            want = _raw_align(d, fresh, "batch", *c)
        assert len(got) == len(c[0]) * d["doubles"] * 8
        assert got == want
        assert (_status(d, got) == 0).any()           # alignments that ran, not a batch of refusals


def test_multi_context_with_an_empty_shard(dims):
    d = dims
    T, S, I = _pairs(d, 2)
    with d["Batch"](**d["kw"]) as b:
        want = _raw_align(d, b, "batch", T, S, I)
    with d["Multi"](devices=[0, 0, 0], **d["kw"]) as m:       # three shards for two pairs: one stays empty
        assert m.device_count == 3
        assert _raw_align(d, m, "multi", T, S, I) == want


def test_tuning_knobs(dims):
    from gtsam_ndt_amd import _lib as L
    d = dims
    with d["Batch"](**d["kw"]) as b:
        for bad in (0, 257):                                  # 1 .. 256 workgroups of the global-table variant
            with pytest.raises(L.NdtError) as e:
                b.set_tuning("batch_global_workgroups", bad)
            assert e.value.code == L.NDT_ERR_INVALID_ARG
        if d["dim"] == 3:                                     # the small variant is 2D's
            with pytest.raises(L.NdtError) as e:
                b.set_tuning("batch_small_variant", 0)
            assert e.value.code == L.NDT_ERR_INVALID_ARG
        else:
            b.set_tuning("batch_small_variant", 0)


def test_3d_context_refuses_overlapping_grids(gpu_lib):
    from gtsam_ndt_amd import _lib as L
    from gtsam_ndt_amd.matcher import NdtBatch3D
    with pytest.raises(L.NdtError) as e:
        NdtBatch3D(overlap_grids=4)
    assert e.value.code == L.NDT_ERR_INVALID_ARG
    assert "overlapping grids are a 2D option" in str(e.value)
