#!/usr/bin/env python3
"""Generates tests/golden/first_launch.npz and tests/golden/first_launch3d.npz: what the alignments of
tests/first_launch_cases.py and tests/first_launch3d_cases.py return on the GPU.

The fixtures pin the results of the single-scan chains bit for bit across the change that folded k_begin / k_begin3
into the first launch of the chain, so they are recorded with the library as it was BEFORE that change and only
regenerated when a change is meant to alter results.  The committed files were written by this script on an MI355X with
NDT_HIP_LIB pointing at libndt_hip.so built from commit 023b5f3 ("Request k_iterate's partial rows ahead of its scalar
batch"), the parent of the commit that added k_iterate_first - not from the fused kernels.  That library does not know
NDT_TUNE_FUSED_BEGIN; the cases are run without touching the knob.  Needs a gfx950 device.  Run from the repo root:
    NDT_HIP_LIB=/path/to/parent/libndt_hip.so python tests/golden/make_first_launch_golden.py [out_dir]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import first_launch_cases as fc          # noqa: E402
import first_launch3d_cases as fc3       # noqa: E402


def record(mod, path):
    world = mod.make_world()
    dev = mod.to_device(world)
    out = {}
    for case in mod.CASES:
        got = mod.run_case(world, dev, case)
        for f in mod.FIELDS:
            out[f"{case[0]}/{f}"] = got[f]
        print(case[0], "iterations", got["iterations"].tolist(), "status", got["status"].tolist(),
              "pose", got["pose"][-1].tolist())
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(mod.CASES)} cases, {os.path.getsize(path)} bytes")


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
    from gtsam_ndt_amd import _lib
    print("recording from", _lib.LIB_PATH)
    record(fc, os.path.join(out_dir, "first_launch.npz"))
    record(fc3, os.path.join(out_dir, "first_launch3d.npz"))


if __name__ == "__main__":
    main()
