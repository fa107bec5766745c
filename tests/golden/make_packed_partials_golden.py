#!/usr/bin/env python3
"""Generates tests/golden/packed_partials.npz: what the alignments, traces and evaluations of
tests/packed_partials_cases.py return on the GPU.

The fixture pins the results of the 2D single-scan chain bit for bit across the change that packed the table between
two launches (AlignDyn::partials: float4[2][3][256] instead of float[2][12][256]), so it is recorded with the library
as it was BEFORE that change and only regenerated when a change is meant to alter results.  The committed file was
written by this script on an MI355X with NDT_HIP_LIB pointing at libndt_hip.so built from commit a29cc2d ("Pin cell
records to an exact reference at degenerate cells (2D, 3D)"), the parent of the commit that packed the table.  Needs a
gfx950 device.  Run from the repo root:
    NDT_HIP_LIB=/path/to/parent/libndt_hip.so python tests/golden/make_packed_partials_golden.py [out_dir]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import packed_partials_cases as pc          # noqa: E402


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden")
    from gtsam_ndt_amd import _lib
    print("recording from", _lib.LIB_PATH)
    world = pc.make_world()
    dev = pc.to_device(world)
    out = {}
    for case in pc.CASES:
        got = pc.run_case(world, dev, case)
        for f in pc.FIELDS:
            out[f"{case[0]}/{f}"] = got[f]
        print(case[0], "iterations", got["iterations"].tolist(), "status", got["status"].tolist(), "n_hit",
              got["n_hit"].tolist(), "pose", got["pose"][-1].tolist())
    path = os.path.join(out_dir, "packed_partials.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {len(pc.CASES)} cases, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
