"""ndt2d/ndt3d_score_particles(_dev, _async) and NDT_TUNE_PARTICLE_TEAM at the ABI: declared in include/ndt_hip.h,
exported, bound in gtsam_ndt_amd/_lib.py, offered by both matchers and both C++ wrappers; the argument error that needs
no device returns its code.  What needs a handle is in test_gpu_score_particles*.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndt_hip.h")
NAMES = [f"ndt{d}d_{f}" for d in (2, 3) for f in ("score_particles_dev", "score_particles_async", "score_particles")]


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
        for p, a in zip(params, args):                      # the scalar arguments sit where the header has them
            if p.startswith("size_t "):
                assert a is C.c_size_t, (name, p)
        dim = int(name[3])
        assert params[0] == f"ndt{dim}d_handle* h"
        assert [p for p in params if p.startswith("size_t ")] == ["size_t n", "size_t m"]
        assert sum(p.startswith("const float*") for p in params) == dim
        assert sum(p.startswith("const double*") for p in params) == 1
        assert params[-2].startswith("float*") and params[-1].startswith("uint32_t*")
        # the three forms of a dimension take the same list of types
        assert [p.split("*")[0] for p in params] == [p.split("*")[0] for p in _prototype(src, f"ndt{dim}d_score_particles_dev")]


def test_the_team_knob_is_declared_and_bound():
    from gtsam_ndt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bNDT_TUNE_PARTICLE_TEAM\s*=\s*(\d+)", src)
    assert m and int(m.group(1)) == 16
    assert _lib.TUNING["particle_team"] == 16
    assert sorted(_lib.TUNING.values()).count(16) == 1
    assert open(HEADER).read().count("NDT_TUNE_PARTICLE_TEAM") >= 4       # the enum, both knob lists, the contract


def test_matchers_and_wrappers_offer_the_calls():
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D, _NdtMatcher
    for cls, coords in ((NdtMatcher2D, ["sx", "sy"]), (NdtMatcher3D, ["sx", "sy", "sz"])):
        sig = inspect.signature(cls.score_particles)
        assert list(sig.parameters) == ["self", *coords, "poses", "with_hits", "sync"]
        assert sig.parameters["with_hits"].default is False and sig.parameters["sync"].default is True
    assert "_score_particles" in vars(_NdtMatcher)                         # the shared code
    import adapter_calls as AC                                  # the C++ adapter's call record
    for method, fn in (("scoreParticlesDev", "score_particles_dev"), ("scoreParticlesAsync", "score_particles_async"),
                       ("scoreParticles", "score_particles")):
        assert AC.both_call(method, fn), method
    for name in NAMES:
        assert name in AC.all_called(), name


def test_a_null_handle_is_an_argument_error(ndt_lib):
    """The one error that needs no device: it is found before any device call."""
    from gtsam_ndt_amd import _lib
    x = np.zeros(4, np.float32)
    poses = np.zeros(12, np.float64)
    out = np.zeros(4, np.float32)
    cnt = np.full(4, 7, np.uint32)
    p, q, o, c = x.ctypes.data, poses.ctypes.data, out.ctypes.data, cnt.ctypes.data
    for name in NAMES:
        scan = (p,) * int(name[3])
        assert getattr(ndt_lib, name)(None, *scan, 4, q, 2, o, c) == _lib.NDT_ERR_INVALID_ARG, name
        assert getattr(ndt_lib, name)(None, *scan, 4, q, 2, o, None) == _lib.NDT_ERR_INVALID_ARG, name
    assert not out.any() and np.all(cnt == 7)
    assert ndt_lib.ndt2d_set_tuning(None, _lib.TUNING["particle_team"], 64) == _lib.NDT_ERR_INVALID_ARG
    assert ndt_lib.ndt3d_set_tuning(None, _lib.TUNING["particle_team"], 64) == _lib.NDT_ERR_INVALID_ARG
