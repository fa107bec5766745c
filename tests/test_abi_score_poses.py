"""ndt2d/ndt3d_score_poses(_dev), _best_poses_dev and _best_poses_align_dev at the ABI: declared in include/ndt_hip.h,
exported, bound in gtsam_ndt_amd/_lib.py, offered by both matchers and both C++ wrappers; the argument error that needs
no device returns its code.  What needs a handle is in test_gpu_score_poses*.py."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndt_hip.h")
NAMES = [f"ndt{d}d_{f}" for d in (2, 3) for f in ("score_poses_dev", "score_poses", "best_poses_dev", "best_poses_align_dev")]


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
        assert [p for p in params if p.startswith("size_t ")] == ["size_t n", "size_t m"]
        assert sum(p.startswith("const float*") for p in params) == dim
        if "best" in name:
            assert f"ndt{dim}d_search_hit* hits" in params and params[-1] == "int32_t* n_hits"
        if "align" in name:
            assert f"ndt{dim}d_result* results" in params


def test_matchers_and_wrappers_offer_the_calls():
    from gtsam_ndt_amd import search
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D, _NdtMatcher
    for cls in (NdtMatcher2D, NdtMatcher3D):
        assert callable(cls.score_poses) and callable(cls.best_poses) and callable(cls.best_poses_align)
    assert "_score_poses" in vars(_NdtMatcher) and "_best_poses" in vars(_NdtMatcher)           # the shared code
    assert callable(search.select_best)
    import adapter_calls as AC                                  # the C++ adapter's call record
    for method, fn in (("scorePosesDev", "score_poses_dev"), ("bestPosesDev", "best_poses_dev"),
                       ("bestPosesAlignDev", "best_poses_align_dev")):
        assert AC.both_call(method, fn), method
    for name in NAMES:
        if name.endswith("_dev"):
            assert name in AC.all_called(), name


def test_a_null_handle_is_an_argument_error(ndt_lib):
    """The one error that needs no device: it is found before any device call."""
    from gtsam_ndt_amd import _lib
    x = np.zeros(4, np.float32)
    poses = np.zeros(12, np.float64)
    out = np.zeros(4, np.float32)
    hits = (_lib.SearchHit3D * 4)()
    res = (_lib.Result3D * 4)()
    nh = C.c_int32(-7)
    p, q, o = x.ctypes.data, poses.ctypes.data, out.ctypes.data
    h, r = C.cast(hits, C.c_void_p), C.cast(res, C.c_void_p)
    calls = {
        "ndt2d_score_poses_dev": (None, p, p, 4, q, 2, o),
        "ndt2d_score_poses": (None, p, p, 4, q, 2, o),
        "ndt2d_best_poses_dev": (None, p, p, 4, q, 2, 0.5, 0.1, 2, h, C.byref(nh)),
        "ndt2d_best_poses_align_dev": (None, p, p, 4, q, 2, 0.5, 0.1, 2, h, r, C.byref(nh)),
        "ndt3d_score_poses_dev": (None, p, p, p, 4, q, 2, o),
        "ndt3d_score_poses": (None, p, p, p, 4, q, 2, o),
        "ndt3d_best_poses_dev": (None, p, p, p, 4, q, 2, 0.5, 0.1, 2, h, C.byref(nh)),
        "ndt3d_best_poses_align_dev": (None, p, p, p, 4, q, 2, 0.5, 0.1, 2, h, r, C.byref(nh)),
    }
    assert sorted(calls) == sorted(NAMES)
    for name, args in calls.items():
        assert getattr(ndt_lib, name)(*args) == _lib.NDT_ERR_INVALID_ARG, name
    assert nh.value == -7 and not out.any()
