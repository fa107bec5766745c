"""The plan of a single-pair launch chain (csrc/ndt_host.hpp: chain_plan) is a pure host rule: fixed and K from the
override and the parameters, whether launch 0 stands in front of the graph, the even chunk of a converged-mode loop, the
length of the graph to fetch.  A stand-alone program compares it, over every combination of override, parameters, knobs
and protocol, with a verbatim copy of the four computations it replaced (2D and 3D, scan and map-to-map), and checks
that chunks are even and that first + launches = K + 1 where the run is not chunked.  Built and run twice, plainly and
with the address and undefined-behaviour sanitizers of the host compiler; it makes no HIP call and needs no GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_include() -> str:
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime.h")):
            return os.path.join(root, "include")
    raise RuntimeError("the HIP headers were not found (ROCM_PATH)")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]],
                         ids=["plain", "sanitized"])
def test_chain_plan_matches_the_four_old_computations(tmp_path, flags):
    exe = tmp_path / "chain_plan_main"
    subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", _hip_include(),
                    "-I", os.path.join(ROOT, "gtsam_ndt_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "chain_plan_main.cpp"),
                    "-o", str(exe), "-ldl"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
