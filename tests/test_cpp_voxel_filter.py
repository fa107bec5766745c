"""The voxel-grid scan filter through the header-only C++ adapter (NdtMatcherHip::voxelFilterDev and the 3D twin):
tests/cpp/voxel_filter_smoke.cpp compiles with plain g++ against the C ABI, makes one call on a matcher without a target
and checks the count and the first and last output point, bit for bit, against what gtsam_ndt_amd/voxel.py computes here.
Without a GPU the program must compile and fail loudly."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory, ndt_lib):
    out = tmp_path_factory.mktemp("cpp") / "voxel_filter_smoke"
    libdir = os.path.join(ROOT, "gtsam_ndt_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "voxel_filter_smoke.cpp"), "-o", str(out),
                    "-L", libdir, "-lndt_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"],
                   check=True)
    return str(out)


def _run(exe, tmp_path, dim, min_points=2):
    from gtsam_ndt_amd import voxel
    pts = np.random.default_rng(40 + dim).uniform(-4.0, 4.0, (1500, dim)).astype(np.float32)
    want, counts = voxel.voxel_filter(pts, 0.3, min_points)
    assert 1 < len(counts) < 1500
    path = str(tmp_path / f"cloud{dim}")
    np.ascontiguousarray(pts.T).tofile(path)
    words = lambda p: [f"{int(w):08x}" for w in p.view(np.uint32)]
    return subprocess.run([exe, str(dim), path, str(len(pts)), "0.3", str(min_points), str(len(counts)), *words(want[0]),
                           *words(want[-1])], capture_output=True, text=True, timeout=120)


def test_program_compiles_and_fails_loudly_without_gpu(exe, tmp_path, ndt_lib):
    if ndt_lib.ndt_device_count() > 0:
        return                                      # (covered by the gpu test)
    r = _run(exe, tmp_path, 2)
    assert r.returncode == 3 and "no CPU fallback" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_one_call_through_the_cpp_adapter(exe, tmp_path, gpu_lib, dim):
    r = _run(exe, tmp_path, dim)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("info 0 ")
