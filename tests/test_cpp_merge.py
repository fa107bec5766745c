"""Submap merging through the header-only C++ adapter (NdtMatcherHip::mergeMap / unmergeMap and the 3D twins): a small
program next to adapter_smoke.cpp loads two saved maps, merges, saves, unmerges, saves; both files must hold the bytes of
tests/map_merge_ref.py.  Without a GPU the program must compile and fail loudly."""
import os
import subprocess

import numpy as np
import pytest

import map_coarsen_ref as R
import map_merge_ref as M
import merge_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory, ndt_lib):
    out = tmp_path_factory.mktemp("cpp") / "merge_smoke"
    libdir = os.path.join(ROOT, "gtsam_ndt_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "merge_smoke.cpp"), "-o", str(out),
                    "-L", libdir, "-lndt_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"],
                   check=True)
    return str(out)


def _blobs(dim):
    """(dst, src) blobs built without the library: the destination a reserved lattice with points of its own."""
    c = MC.C2 if dim == 2 else MC.C3
    lo, hi = MC.extent(dim, "tiny", 2.0)
    origin, ext = MC.reserved_geometry(dim, lo, hi, c)
    own = MC.own_points(dim, "tiny")
    if dim == 2:                                    # (ndt2d_load_map clears the ring: keep the points off it)
        idx = R.blob_from_points(own, c, origin, ext)[1]
        own = own[np.all((idx >= 1) & (idx < np.array(ext) - 1), axis=1)]
    return R.blob_from_points(own, c, origin, ext)[0], R.blob_from_points(MC.points(dim, "tiny"), c)[0]


def _run(exe, tmp_path, dim, pose_name="general"):
    dst, src = _blobs(dim)
    pose = MC.poses(dim, "tiny")[pose_name]
    paths = [str(tmp_path / f"{k}{dim}.map") for k in ("dst", "src", "merged", "back")]
    dst.tofile(paths[0])
    src.tofile(paths[1])
    r = subprocess.run([exe, str(dim), *paths, *[repr(float(v)) for v in pose]], capture_output=True, text=True, timeout=120)
    return dst, src, pose, paths, r


def test_merge_program_compiles_and_fails_loudly_without_gpu(exe, tmp_path, ndt_lib):
    if ndt_lib.ndt_device_count() > 0:
        return                                      # (covered by the gpu test)
    *_, r = _run(exe, tmp_path, 2)
    assert r.returncode == 3 and "no CPU fallback" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_merge_through_the_cpp_adapter(exe, tmp_path, gpu_lib, dim):
    _merge_through_the_cpp_adapter(exe, tmp_path, dim, "general")


@pytest.mark.gpu
@pytest.mark.parametrize("pose_name", MC.TILTED)
def test_merge_through_the_cpp_adapter_at_tilted_poses(exe, tmp_path, gpu_lib, pose_name):
    _merge_through_the_cpp_adapter(exe, tmp_path, 3, pose_name)


def _merge_through_the_cpp_adapter(exe, tmp_path, dim, pose_name):
    dst, src, pose, paths, r = _run(exe, tmp_path, dim, pose_name)
    assert r.returncode == 0, r.stdout + r.stderr
    want, want_out = M.map_merge_ref(dst, src, pose)
    assert r.stdout.split() == ["outside", str(want_out), str(want_out)]
    assert np.array_equal(np.fromfile(paths[2], dtype=np.uint8), want)
    assert np.array_equal(np.fromfile(paths[3], dtype=np.uint8), dst)
