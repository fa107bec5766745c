"""ndt2d/ndt3d_remove_target_points(_dev): declared in include/ndt_hip.h, exported by the library and bound in
gtsam_ndt_amd/_lib.py with the argument types of their add twins; the matchers offer remove_target_points() beside
add_target_points().  Needs no device."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndt_hip.h")

PAIRS = [("ndt2d_remove_target_points", "ndt2d_add_target_points"),
         ("ndt2d_remove_target_points_dev", "ndt2d_add_target_points_dev"),
         ("ndt3d_remove_target_points", "ndt3d_add_target_points"),
         ("ndt3d_remove_target_points_dev", "ndt3d_add_target_points_dev")]


def _prototype(src, name):
    m = re.search(r"\bint32_t\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in ndt_hip.h"
    return re.sub(r"\s+", " ", m.group(1)).strip()


def test_remove_symbols_are_declared_exported_and_bound_like_their_add_twins(ndt_lib):
    from gtsam_ndt_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for remove, add in PAIRS:
        assert _prototype(src, remove) == _prototype(src, add), (remove, add)       # the same parameter list, names included
        assert hasattr(ndt_lib, remove), f"{remove} is not exported"
        assert remove in _lib.SIGNATURES, f"{remove} is not bound"
        assert _lib.SIGNATURES[remove] == _lib.SIGNATURES[add], (remove, add)
        fn = getattr(ndt_lib, remove)
        assert fn.restype is _lib.SIGNATURES[add][0] and list(fn.argtypes) == list(_lib.SIGNATURES[add][1])
    assert ndt_lib.ndt_abi_version() == 1


def test_matchers_offer_remove_beside_add():
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D
    for cls in (NdtMatcher2D, NdtMatcher3D):
        add, remove = inspect.signature(cls.add_target_points), inspect.signature(cls.remove_target_points)
        assert list(add.parameters) == list(remove.parameters)
        assert remove.parameters["pose"].default is None


def test_cpp_wrapper_has_the_remove_twins():
    import adapter_calls as AC                                  # the C++ adapter's call record
    assert AC.both_call("removeTargetPoints", "remove_target_points")
    assert AC.both_call("removeTargetPointsDev", "remove_target_points_dev")
    # ... and nothing but them: the remove twins call what their add twins call, with "remove" for "add"
    for cls in ("NdtMatcherHip", "NdtMatcherHip3"):
        for m in ("TargetPoints", "TargetPointsDev"):
            add, remove = AC.calls()[f"{cls}.add{m}"], AC.calls()[f"{cls}.remove{m}"]
            assert [f.replace("_add_", "_remove_") for f in add] == remove, (cls, m)
