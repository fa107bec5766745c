"""ndt2d/ndt3d_score_map_poses(_dev), _best_map_poses_dev and _best_map_poses_align_dev at the ABI: declared in
include/ndt_hip.h, exported, bound in gtsam_ndt_amd/_lib.py, offered by both matchers and both C++ wrappers; the argument
errors that need no device return their codes.  What needs a handle is in test_gpu_score_map_poses*.py."""
import ctypes as C
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndt_hip.h")
FUNCS = ("score_map_poses_dev", "score_map_poses", "best_map_poses_dev", "best_map_poses_align_dev")
NAMES = [f"ndt{d}d_{f}" for d in (2, 3) for f in FUNCS]


def _prototype(src, name):
    m = re.search(r"\bint32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in ndt_hip.h"
    return [p.strip() for p in re.sub(r"\s+", " ", m.group(1)).split(",")]


def test_symbols_are_declared_exported_and_bound(ndt_lib):
    from gtsam_ndt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in NAMES:
        params = _prototype(src, name)
        assert hasattr(ndt_lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int32 and len(args) == len(params), name
        fn = getattr(ndt_lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
        # the scalar arguments sit where the header has them
        for p, a in zip(params, args):
            if p.startswith("size_t "):
                assert a is C.c_size_t, (name, p)
            if p.startswith("double min_sep"):
                assert a is C.c_double, (name, p)
            if p.startswith("int32_t k"):
                assert a is C.c_int32, (name, p)
            if p.startswith("int32_t* n_hits"):
                assert a == C.POINTER(C.c_int32), (name, p)
        dim = int(name[3])
        assert params[:2] == [f"ndt{dim}d_handle* target", f"ndt{dim}d_handle* source"]
        assert params[2].startswith("const double*") and params[3] == "size_t m"
        assert [p for p in params if p.startswith("size_t ")] == ["size_t m"]
        if "score" in name:
            assert params[4].startswith("float*") and params[5].startswith("uint32_t*") and len(params) == 6
        if "best" in name:
            assert params[4:7] == ["double min_sep_trans", "double min_sep_rot", "int32_t k"]
            assert params[7] == f"ndt{dim}d_search_hit* hits" and params[-1] == "int32_t* n_hits"
        if "align" in name:
            assert params[8] == f"ndt{dim}d_result* results"


def test_matchers_and_wrappers_offer_the_calls():
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D, _NdtMatcher
    for cls in (NdtMatcher2D, NdtMatcher3D):
        assert callable(cls.score_map_poses) and callable(cls.best_map_poses) and callable(cls.best_map_poses_align)
    for shared in ("score_map_poses", "best_map_poses", "best_map_poses_align"):           # the shared code
        assert shared in vars(_NdtMatcher)
    import adapter_calls as AC                                  # the C++ adapter's call record
    for method, fn in (("scoreMapPosesDev", "score_map_poses_dev"), ("bestMapPosesDev", "best_map_poses_dev"),
                       ("bestMapPosesAlignDev", "best_map_poses_align_dev")):
        assert AC.both_call(method, fn), method
    for name in NAMES:
        if name.endswith("_dev"):
            assert name in AC.all_called(), name


def test_argument_errors_are_found_without_a_device(ndt_lib):
    """Null pointers, m = 0, k outside 1..64 and a bad separation are refused before either handle is looked at: the
    handles here are not handles at all (no call reads them), so no device is needed.  *n_hits is 0 wherever it could
    be written; the outputs are untouched."""
    from gtsam_ndt_amd import _lib
    INV = _lib.NDT_ERR_INVALID_ARG
    poses = np.zeros(12, np.float64)
    out = np.zeros(4, np.float32)
    cnt = np.zeros(4, np.uint32)
    hits = (_lib.SearchHit3D * 64)()
    res = (_lib.Result3D * 64)()
    q, o, c = poses.ctypes.data, out.ctypes.data, cnt.ctypes.data
    h, r = C.cast(hits, C.c_void_p), C.cast(res, C.c_void_p)
    fake = C.cast(C.create_string_buffer(64), C.c_void_p)      # stands for a handle in calls refused before it is read
    for dim in (2, 3):
        f = {name: getattr(ndt_lib, f"ndt{dim}d_{name}") for name in FUNCS}
        for score in (f["score_map_poses_dev"], f["score_map_poses"]):
            assert score(None, None, q, 2, o, c) == INV
            assert score(None, fake, q, 2, o, c) == INV and score(fake, None, q, 2, o, c) == INV
            assert score(fake, fake, None, 2, o, c) == INV and score(fake, fake, q, 2, None, c) == INV
            assert score(fake, fake, q, 0, o, c) == INV and score(fake, fake, q, 0, o, None) == INV
            assert score(fake, fake, q, 2 ** 25 + 1, o, c) == _lib.NDT_ERR_CAPACITY
            assert b"2^25" in ndt_lib.ndt_last_error()

        def best(t=fake, s=fake, p=q, m=2, sep=(0.5, 0.1), k=2, hp=h, nh=None, align=False, rp=r):
            tail = (C.byref(nh) if nh is not None else None,)
            if align:
                return f["best_map_poses_align_dev"](t, s, p, m, sep[0], sep[1], k, hp, rp, *tail)
            return f["best_map_poses_dev"](t, s, p, m, sep[0], sep[1], k, hp, *tail)

        for align in (False, True):
            for kw in (dict(t=None), dict(s=None), dict(p=None), dict(m=0), dict(hp=None), dict(k=0), dict(k=65), dict(k=-1),
                       dict(sep=(math.nan, 0.1)), dict(sep=(0.5, math.inf)), dict(sep=(-0.5, 0.1)), dict(sep=(0.5, -0.1))):
                nh = C.c_int32(-7)
                assert best(nh=nh, align=align, **kw) == INV, (dim, align, kw)
                assert nh.value == 0, (dim, align, kw)
            assert best(nh=None, align=align) == INV
        nh = C.c_int32(-7)
        assert best(nh=nh, align=True, rp=None) == INV and nh.value == 0
    assert not out.any() and not cnt.any()
