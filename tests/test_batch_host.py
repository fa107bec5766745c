"""The device-free half of the batch and multi-device contexts (csrc/ndt_host.hpp: the validation of a batch's pair
offsets, the split of the pairs into shards, the rebasing of a shard's offsets, the layout of the result gather) is
made of pure host functions: a stand-alone program walks them.  Built with the address and undefined-behaviour
sanitizers of the host compiler; it makes no HIP call and needs no GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hip_include() -> str:
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime.h")):
            return os.path.join(root, "include")
    raise RuntimeError("the HIP headers were not found (ROCM_PATH)")


def test_the_host_logic_of_the_batch_contexts(tmp_path):
    exe = tmp_path / "batch_host_test"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-isystem", _hip_include(),
                    "-I", os.path.join(ROOT, "gtsam_ndt_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "batch_host_test.cpp"), "-o", str(exe), "-ldl"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
