"""ndt3d_set_neighbourhood / ndt3d_neighbourhood at the ABI, where no device is needed: declared in include/ndt_hip.h,
exported, bound in gtsam_ndt_amd/_lib.py; a null handle is NDT_ERR_INVALID_ARG; the option is a call, not a field:
ndt3d_params keeps its 104 bytes and NDT_ABI_VERSION stays 1."""
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
    assert re.search(r"\bint32_t\s+ndt3d_set_neighbourhood\s*\(\s*ndt3d_handle\s*\*\s*h\s*,\s*int32_t\s+n\s*\)\s*;", src)
    assert re.search(r"\bint32_t\s+ndt3d_neighbourhood\s*\(\s*const\s+ndt3d_handle\s*\*\s*h\s*\)\s*;", src)
    for name, args in (("ndt3d_set_neighbourhood", [C.c_void_p, C.c_int32]), ("ndt3d_neighbourhood", [C.c_void_p])):
        assert hasattr(ndt_lib, name), f"{name} is not exported"
        assert _lib.SIGNATURES[name] == (C.c_int32, args)
        fn = getattr(ndt_lib, name)
        assert fn.restype is C.c_int32 and list(fn.argtypes) == args


def test_a_null_handle_is_an_argument_error(ndt_lib):
    from gtsam_ndt_amd import _lib
    for n in (1, 7, 3):
        assert ndt_lib.ndt3d_set_neighbourhood(None, n) == _lib.NDT_ERR_INVALID_ARG
        assert "ndt3d_set_neighbourhood" in ndt_lib.ndt_last_error().decode()
    assert ndt_lib.ndt3d_neighbourhood(None) == _lib.NDT_ERR_INVALID_ARG


def test_the_abi_version_and_the_params_struct_are_unchanged(ndt_lib, tmp_path):
    from gtsam_ndt_amd import _lib
    assert ndt_lib.ndt_abi_version() == 1
    assert C.sizeof(_lib.Params2D) == 104
    assert [f[0] for f in _lib.Params2D._fields_][-4:] == ["overlap_grids", "line_search", "reserved", "step_scale"]
    src = tmp_path / "size.c"
    src.write_text('#include "ndt_hip.h"\n_Static_assert(sizeof(ndt3d_params) == 104, "ndt3d_params");\n'
                   '_Static_assert(sizeof(ndt2d_params) == 104, "ndt2d_params");\n'
                   '_Static_assert(NDT_ABI_VERSION == 1, "abi");\nint main(void) { return 0; }\n')
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-fsyntax-only", str(src)], check=True)


def test_the_3d_classes_take_the_keyword():
    """A keyword of the 3D classes, not a parameter override (the params struct has no such field)."""
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D, NdtPyramid2D, NdtPyramid3D
    for cls in (NdtMatcher3D, NdtPyramid3D):
        assert inspect.signature(cls.__init__).parameters["neighbourhood"].default == 1
    for cls in (NdtMatcher2D, NdtPyramid2D):
        assert "neighbourhood" not in inspect.signature(cls.__init__).parameters
    assert callable(NdtMatcher3D.set_neighbourhood) and isinstance(NdtMatcher3D.neighbourhood, property)
    assert not hasattr(NdtMatcher2D, "set_neighbourhood")
