"""ndt3d_align_map_multi checks its pointers and the number of starts before it makes any device call, so these rows of
its error table hold on a machine without a GPU; and the Python binding exists."""
import ctypes as C

import pytest

from gtsam_ndt_amd import _lib as L


def _args():
    """Non-null stand-ins: none of them may be looked into before the checks below have returned."""
    handle = C.create_string_buffer(64)
    sources = (C.c_void_p * 64)(*[C.addressof(handle)] * 64)
    poses = (C.c_double * (6 * 64))()
    results = (L.Result3D * 64)()
    return handle, sources, poses, results


@pytest.mark.parametrize("null", ["target", "sources", "init_poses", "results"])
def test_null_pointers_are_invalid_arguments(ndt_lib, null):
    handle, sources, poses, results = _args()
    args = dict(target=C.addressof(handle), sources=C.cast(sources, C.c_void_p), init_poses=C.cast(poses, C.c_void_p),
                results=C.cast(results, C.c_void_p))
    args[null] = None
    assert ndt_lib.ndt3d_align_map_multi(args["target"], args["sources"], args["init_poses"], 2,
                                         args["results"]) == L.NDT_ERR_INVALID_ARG


@pytest.mark.parametrize("m", [0, 65, -1])
def test_the_number_of_starts_is_checked_first(ndt_lib, m):
    handle, sources, poses, results = _args()
    assert ndt_lib.ndt3d_align_map_multi(C.addressof(handle), C.cast(sources, C.c_void_p), C.cast(poses, C.c_void_p), m,
                                         C.cast(results, C.c_void_p)) == L.NDT_ERR_INVALID_ARG


def test_a_null_entry_of_sources_is_an_invalid_argument(ndt_lib):
    handle, sources, poses, results = _args()
    sources[1] = None
    assert ndt_lib.ndt3d_align_map_multi(C.addressof(handle), C.cast(sources, C.c_void_p), C.cast(poses, C.c_void_p), 3,
                                         C.cast(results, C.c_void_p)) == L.NDT_ERR_INVALID_ARG


def test_the_matcher_has_the_call():
    from gtsam_ndt_amd.matcher import NdtMatcher3D
    assert callable(getattr(NdtMatcher3D, "align_map_multi"))
    assert "map_multi_from" in L.TUNING
