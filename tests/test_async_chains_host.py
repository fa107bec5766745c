"""The rotation and fork rule of a handle's launch chains at 1..4 lanes (csrc/ndt_host.hpp: lane_step) is a pure host
rule: a stand-alone program checks the exact sequences at three and four lanes and a model of the streams (ordered
queues, event record and wait edges) over random event sequences, against a verbatim copy of the two-lane rule where
the count is 1 or 2.  Built and run twice, plainly and with the address and undefined-behaviour sanitizers of the host
compiler; it makes no HIP call and needs no GPU."""
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
def test_lane_rule_up_to_four_lanes(tmp_path, flags):
    exe = tmp_path / "lanes_n_host_test"
    subprocess.run(["g++", "-std=c++17", *flags, "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", "-isystem", _hip_include(),
                    "-I", os.path.join(ROOT, "gtsam_ndt_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "lanes_n_host_test.cpp"),
                    "-o", str(exe), "-ldl"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
