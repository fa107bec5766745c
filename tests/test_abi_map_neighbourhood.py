"""ndt3d_set_map_neighbourhood / ndt3d_map_neighbourhood at the ABI, where no device is needed (the twin of
tests/test_abi_neighbourhood.py): declared in include/ndt_hip.h, exported, bound in gtsam_ndt_amd/_lib.py; a null handle
is NDT_ERR_INVALID_ARG with the function named; the option is a call, not a field: ndt3d_params keeps its 104 bytes and
NDT_ABI_VERSION stays 1; the 3D Python classes take the keyword, the 2D classes do not."""
import ctypes as C
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndt_hip.h")


def test_symbols_are_declared_exported_and_bound(ndt_lib):
    from gtsam_ndt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint32_t\s+ndt3d_set_map_neighbourhood\s*\(\s*ndt3d_handle\s*\*\s*h\s*,\s*int32_t\s+n\s*\)\s*;", src)
    assert re.search(r"\bint32_t\s+ndt3d_map_neighbourhood\s*\(\s*const\s+ndt3d_handle\s*\*\s*h\s*\)\s*;", src)
    assert not re.search(r"ndt2d_\w*map_neighbourhood", src)
    for name, args in (("ndt3d_set_map_neighbourhood", [C.c_void_p, C.c_int32]), ("ndt3d_map_neighbourhood", [C.c_void_p])):
        assert hasattr(ndt_lib, name), f"{name} is not exported"
        assert _lib.SIGNATURES[name] == (C.c_int32, args)
        fn = getattr(ndt_lib, name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == args
    assert not hasattr(ndt_lib, "ndt2d_set_map_neighbourhood")


def test_a_null_handle_is_an_argument_error(ndt_lib):
    from gtsam_ndt_amd import _lib
    for n in (1, 7, 3):
        assert ndt_lib.ndt3d_set_map_neighbourhood(None, n) == _lib.NDT_ERR_INVALID_ARG
        assert "ndt3d_set_map_neighbourhood" in ndt_lib.ndt_last_error().decode()
    assert ndt_lib.ndt3d_map_neighbourhood(None) == _lib.NDT_ERR_INVALID_ARG
    assert "ndt3d_map_neighbourhood" in ndt_lib.ndt_last_error().decode()


def test_the_abi_version_and_the_params_structs_are_unchanged(ndt_lib, tmp_path):
    from gtsam_ndt_amd import _lib
    assert ndt_lib.ndt_abi_version() == 1
    assert C.sizeof(_lib.Params2D) == 104                           # the binding's one struct for ndt2d_params and ndt3d_params
    assert "neighbourhood" not in " ".join(f[0] for f in _lib.Params2D._fields_)
    src = tmp_path / "size.c"
    src.write_text('#include "ndt_hip.h"\n_Static_assert(sizeof(ndt3d_params) == 104, "ndt3d_params");\n'
                   '_Static_assert(sizeof(ndt2d_params) == 104, "ndt2d_params");\n'
                   '_Static_assert(NDT_ABI_VERSION == 1, "abi");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_the_3d_classes_take_the_keyword():
    """A keyword of the 3D classes, not a parameter override (the params struct has no such field)."""
    from gtsam_ndt_amd.matcher import NdtMapPyramid2D, NdtMapPyramid3D, NdtMatcher2D, NdtMatcher3D
    for cls in (NdtMatcher3D, NdtMapPyramid3D):
        assert inspect.signature(cls.__init__).parameters["map_neighbourhood"].default == 1
    assert inspect.signature(NdtMapPyramid3D.from_blob).parameters["map_neighbourhood"].default == 1
    for cls in (NdtMatcher2D, NdtMapPyramid2D):
        assert "map_neighbourhood" not in inspect.signature(cls.__init__).parameters
    assert callable(NdtMatcher3D.set_map_neighbourhood) and isinstance(NdtMatcher3D.map_neighbourhood, property)
    assert not hasattr(NdtMatcher2D, "set_map_neighbourhood") and not hasattr(NdtMatcher2D, "map_neighbourhood")
    # a setting of its own, next to the point neighbourhood
    assert inspect.signature(NdtMatcher3D.__init__).parameters["neighbourhood"].default == 1
