"""Sweep de-skewing through the header-only C++ adapter (include/ndt_matcher_hip.hpp): tests/cpp/deskew_smoke.cpp compiles
with plain g++ against the C ABI; sweepMotion needs no device and equals the ctypes binding to the bit; on the GPU the
de-skewing overloads of the two conversions and deskewPointsDev give the bits the Python binding gives."""
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREV, CUR = (1.0, 2.0, 0.5, 0.1, -0.2, 0.3), (1.4, 2.1, 0.45, 0.12, -0.18, 0.42)
MOTION2, MOTION3 = (0.25, 0.05, 0.08), (0.5, 0.1, 0.02, 0.01, -0.01, 0.12)


@pytest.fixture(scope="module")
def exe(tmp_path_factory, ndt_lib):
    out = tmp_path_factory.mktemp("cpp") / "deskew_smoke"
    libdir = os.path.join(ROOT, "gtsam_ndt_amd", "lib")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "deskew_smoke.cpp"), "-o", str(out),
                    "-L", libdir, "-lndt_hip", f"-Wl,-rpath,{libdir}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib",
                    "-lamdhip64"],
                   check=True)
    return str(out)


def test_sweep_motion_through_the_adapter(exe, ndt_lib):
    from gtsam_ndt_amd.matcher import sweep_motion
    r = subprocess.run([exe, "host", *[repr(v) for v in PREV + CUR]], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = dict((l.split()[0], l.split()[1:]) for l in r.stdout.strip().splitlines())
    assert tuple(float.fromhex(v) for v in lines["sweep3"]) == sweep_motion(PREV, CUR)
    two = lambda p: (p[0], p[1], p[5])
    assert tuple(float.fromhex(v) for v in lines["sweep2"]) == sweep_motion(two(PREV), two(CUR))
    assert lines["refused"] == ["-1"]


@pytest.mark.gpu
def test_device_calls_through_the_adapter(exe, tmp_path, gpu_lib):
    import torch
    from gtsam_ndt_amd.matcher import deskew_points, polar_to_points, range_image_to_points
    rng = np.random.default_rng(11)
    n, ne, na = 1000, 5, 300
    r2 = rng.uniform(0.5, 100.0, n).astype(np.float32)
    r3 = rng.uniform(0.5, 100.0, (ne, na)).astype(np.float32)
    r2[3], r3[1, 7] = np.nan, 500.0
    f2 = rng.uniform(-0.25, 1.25, n).astype(np.float32)
    f3 = rng.uniform(-0.25, 1.25, ne * na).astype(np.float32)
    el = np.deg2rad(np.linspace(-24.0, 20.0, ne))
    files = {}
    for name, a in (("r2", r2), ("f2", f2), ("r3", r3), ("f3", f3), ("el", el)):
        files[name] = str(tmp_path / name)
        a.tofile(files[name])
    out = str(tmp_path / "out.f32")
    r = subprocess.run([exe, "dev", files["r2"], files["f2"], str(n), files["r3"], files["f3"], files["el"], str(ne), str(na), out],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(out, dtype=np.float32)
    cuda = lambda a: torch.from_numpy(a).cuda()
    inc = 2.0 * math.pi / n
    a = polar_to_points(cuda(r2), -math.pi + 0.5 * inc, inc, 0.05, 100.0, motion=MOTION2, frac=(-0.25, 1.5 / n), ref_frac=0.5)
    b = deskew_points(a, cuda(f2), MOTION2, 1.0)
    inc = 2.0 * math.pi / na
    c = range_image_to_points(cuda(r3), el, -math.pi + 0.5 * inc, inc, 0.05, 100.0, motion=MOTION3, frac=(-0.25, 1.5 / na),
                              ref_frac=0.5)
    d = deskew_points(c, cuda(f3), MOTION3, 1.0)
    want = np.concatenate([t.cpu().numpy() for t in (*a, *b, *c, *d)])
    assert got.size == want.size and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(got[3]) and np.isfinite(got[4]) and np.isnan(got[4 * n + na + 7])
