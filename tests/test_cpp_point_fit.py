"""Per-point fit and selection through the header-only C++ adapter (NdtMatcherHip::fitPointsDev / selectPointsDev and
the 3D twins): a small program next to merge_smoke.cpp loads a saved map and a scan, calls both wrappers and the C
functions on a second handle of the same map; the summaries must be equal to each other and to the Python matcher's, and
the classes and indices the wrapper left on the device equal to the matcher's.  Without a GPU the program must compile
and fail loudly."""
import os
import subprocess

import numpy as np
import pytest

import point_fit_cases as PC
import point_fit_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEEP = (1 << F.FIT) | (1 << F.MISS)


@pytest.fixture(scope="module")
def exe(tmp_path_factory, ndt_lib):
    out = tmp_path_factory.mktemp("cpp") / "point_fit_smoke"
    libdir = os.path.join(ROOT, "gtsam_ndt_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "point_fit_smoke.cpp"), "-o", str(out),
                    "-L", libdir, "-lndt_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"],
                   check=True)
    return str(out)


def _run(exe, tmp_path, dim, blob, scan, pose):
    paths = [str(tmp_path / f"{k}{dim}") for k in ("map", "scan", "classes", "index")]
    np.ascontiguousarray(blob).tofile(paths[0])
    np.concatenate([np.asarray(c, dtype=np.float32) for c in scan]).tofile(paths[1])
    return paths, subprocess.run([exe, str(dim), paths[0], paths[1], str(len(scan[0])), repr(PC.MAX_M[dim]), str(KEEP), paths[2],
                                  paths[3], *[repr(float(v)) for v in pose]], capture_output=True, text=True, timeout=120)


def test_program_compiles_and_fails_loudly_without_gpu(exe, tmp_path, ndt_lib):
    if ndt_lib.ndt_device_count() > 0:
        return                                      # (covered by the gpu test)
    import map_coarsen_ref as R
    fx = PC.fixture(2)
    blob = R.blob_from_points(np.stack(fx["target"], axis=1), 0.5)[0]
    _, r = _run(exe, tmp_path, 2, blob, fx["source"], fx["final_pose"])
    assert r.returncode == 3 and "no CPU fallback" in r.stdout


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [2, 3])
def test_fit_and_select_through_the_cpp_adapter(exe, tmp_path, gpu_lib, dim):
    fx = PC.fixture(dim)
    pose = fx["final_pose"]
    with PC.matcher(dim) as m:
        rec = F.records_of(m)
        scan, _ = PC.mixed_scan(rec, fx["source"], pose, 2500)
        want = m.fit_points(*scan, pose, PC.MAX_M[dim])
        _, idx, sel = m.select_points(*scan, pose, PC.MAX_M[dim], keep=KEEP)
        paths, r = _run(exe, tmp_path, dim, m.save_map(), scan, pose)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {ln.split()[0]: tuple(int(v) for v in ln.split()[1:]) for ln in r.stdout.splitlines()}
    counts = (want.n_invalid, want.n_miss, want.n_misfit, want.n_fit)
    assert rows["wrapper_fit"] == rows["c_fit"] == counts + (0,)
    assert rows["wrapper_select"] == rows["c_select"] == counts + (sel.n_selected,) and sel.n_selected == len(idx) > 0
    assert np.array_equal(np.fromfile(paths[2], dtype=np.uint8), want.cls)
    assert np.array_equal(np.fromfile(paths[3], dtype=np.uint32).astype(np.int64), idx)
