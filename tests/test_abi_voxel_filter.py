"""ndt2d/ndt3d_voxel_filter(_dev) at the ABI: declared in include/ndt_hip.h, exported, bound in gtsam_ndt_amd/_lib.py;
sizeof(ndt_voxel_filter_info) equals the ctypes mirror (a compiled C program says so); every argument error is found
before the device or the handle is touched and returns its code with a message in ndt_last_error; without a device a
well-formed call returns the library's no-device error.  What needs a device is in test_gpu_voxel_filter.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ndt_hip.h")
NAMES = [f"ndt{d}d_{f}" for d in (2, 3) for f in ("voxel_filter_dev", "voxel_filter")]


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
        for p, a in zip(params, args):                          # the scalar arguments sit where the header has them
            if p.startswith("double leaf"):
                assert a is C.c_double
            if p.startswith("uint32_t min_points"):
                assert a is C.c_uint32
            if p.startswith("size_t "):
                assert a is C.c_size_t
        assert params[-1] == "ndt_voxel_filter_info* info" and args[-1] == C.POINTER(_lib.VoxelFilterInfo)
        assert len(params) == (11 if name.startswith("ndt2d") else 13)
    assert ndt_lib.ndt_abi_version() == 1


def test_the_info_struct_matches_its_mirror(tmp_path):
    from gtsam_ndt_amd import _lib
    assert [f[0] for f in _lib.VoxelFilterInfo._fields_] == ["n_invalid", "n_voxels", "n_out"]
    prog = tmp_path / "size.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "ndt_hip.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu\\n", sizeof(ndt_voxel_filter_info), offsetof(ndt_voxel_filter_info, n_invalid),'
                    ' offsetof(ndt_voxel_filter_info, n_voxels), offsetof(ndt_voxel_filter_info, n_out)); return 0;}\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    I = _lib.VoxelFilterInfo
    assert out == [C.sizeof(I), I.n_invalid.offset, I.n_voxels.offset, I.n_out.offset] == [24, 0, 8, 16]


def test_matchers_and_wrappers_offer_the_calls():
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D, _NdtMatcher
    for cls in (NdtMatcher2D, NdtMatcher3D):
        assert callable(cls.voxel_filter)
    assert "_voxel_filter" in vars(_NdtMatcher)                 # the shared code
    import adapter_calls as AC                                  # the C++ adapter's call record
    assert AC.both_call("voxelFilterDev", "voxel_filter_dev")
    for name in NAMES:
        if name.endswith("_dev"):
            assert name in AC.all_called(), name


def _call(lib, dim, host, h, n=4, leaf=0.25, min_points=1, null_in=None, null_out=None, info=True, overlap=None, capacity=4):
    """One call with host arrays standing for whichever memory the entry takes: every call here is refused before any
    array is read.  -> (status, message, info, keep-alive)."""
    from gtsam_ndt_amd import _lib
    src = [np.zeros(8, np.float32) for _ in range(dim)]
    out = [np.zeros(8, np.float32) for _ in range(dim)]
    cnt = np.zeros(8, np.uint32)
    s = [None if a == null_in else c.ctypes.data for a, c in enumerate(src)]
    o = [None if a == null_out else c.ctypes.data for a, c in enumerate(out)]
    c = cnt.ctypes.data
    if overlap == "out":
        o[dim - 1] = src[0].ctypes.data + 4 * (n - 1)           # its first element is the input's last
    if overlap == "count":
        c = src[dim - 1].ctypes.data
    fi = _lib.VoxelFilterInfo(7, 7, 7)
    fn = getattr(lib, f"ndt{dim}d_voxel_filter" + ("" if host else "_dev"))
    st = fn(h, *s, n, leaf, min_points, *o, c, capacity, C.byref(fi) if info else None)
    return st, lib.ndt_last_error().decode(), fi, (src, out, cnt)


def test_argument_errors_are_found_before_the_device(ndt_lib):
    from gtsam_ndt_amd import _lib
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)    # stands for a handle in calls refused before it is read
    nan, inf = float("nan"), float("inf")
    cases = [("handle", dict(h=None)), ("input", dict(null_in=0)), ("output", dict(null_out=0)), ("info", dict(info=False)),
             ("empty", dict(n=0)), ("more points", dict(n=2 ** 31)), ("leaf", dict(leaf=0.0)), ("leaf", dict(leaf=-0.25)),
             ("leaf", dict(leaf=nan)), ("leaf", dict(leaf=inf)), ("min_points", dict(min_points=0)),
             ("overlaps", dict(overlap="out")), ("overlaps", dict(overlap="count"))]
    for dim in (2, 3):
        for host in (False, True):
            name = f"ndt{dim}d_voxel_filter" + ("" if host else "_dev")
            for word, kw in cases + [("input", dict(null_in=dim - 1)), ("output", dict(null_out=dim - 1))]:
                kw = dict(kw)
                st, msg, fi, _ = _call(ndt_lib, dim, host, kw.pop("h", fake), **kw)
                assert st == _lib.NDT_ERR_INVALID_ARG, (name, word, kw, st)
                assert msg.startswith(name + ":") and word in msg, (name, word, msg)
                assert (fi.n_invalid, fi.n_voxels, fi.n_out) == (7, 7, 7)         # a refused call writes nothing


def test_without_a_device_a_good_call_is_the_no_device_error(ndt_lib):
    """Where there is no device no handle can exist, so a block of zeros stands for one: the call must answer before it
    reads it.  Where there is a device the same call, on a real handle, is served."""
    from gtsam_ndt_amd import _lib
    for dim in (2, 3):
        for host in (False, True):
            if ndt_lib.ndt_device_count() > 0:
                if not host:
                    continue                                    # (device arrays: test_gpu_voxel_filter.py)
                from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D
                with (NdtMatcher2D() if dim == 2 else NdtMatcher3D()) as m:
                    st, msg, fi, _ = _call(ndt_lib, dim, host, m._h)
                assert st == 0 and (fi.n_invalid, fi.n_voxels, fi.n_out) == (0, 1, 1)
                continue
            fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
            st, msg, fi, _ = _call(ndt_lib, dim, host, fake)
            assert st == _lib.NDT_ERR_NO_DEVICE, (dim, host, st, msg)
            assert "no HIP device" in msg and "voxel_filter" in msg
            assert (fi.n_invalid, fi.n_voxels, fi.n_out) == (0, 0, 0)
