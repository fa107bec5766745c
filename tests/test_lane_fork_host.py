"""When lane 1 of a handle forks from the handle's stream (csrc/ndt_host.hpp: lane_step's `mark` and `wait`) is a pure
host rule: a stand-alone program checks the exact sequences and an ordering model over random event sequences.  Built
with the address and undefined-behaviour sanitizers of the host compiler; it makes no HIP call and needs no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_include() -> str:
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime.h")):
            return os.path.join(root, "include")
    raise RuntimeError("the HIP headers were not found (ROCM_PATH)")


def test_lane_fork_rule(tmp_path):
    exe = tmp_path / "lane_fork_host_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-isystem", _hip_include(),
                    "-I", os.path.join(ROOT, "gtsam_ndt_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "lane_fork_host_test.cpp"),
                    "-o", str(exe), "-ldl"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
