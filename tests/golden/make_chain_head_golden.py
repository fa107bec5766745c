#!/usr/bin/env python3
"""Generates tests/golden/chain_head.npz: what the alignments of tests/chain_head_cases.py return on the GPU.

The fixture pins k_iterate's results bit for bit across changes that may only reorder its loads and waits, so it is
recorded with the library as it was BEFORE such a change and only regenerated when a change is meant to alter results.
The committed file was written by this script on an MI355X with NDT_HIP_LIB pointing at libndt_hip.so built from
commit c582b6a ("Align up to 64 3D map-to-map problems against one target per chain"), the parent of the commit that
reordered the head of the launch - not from the reordered kernels.  Needs a gfx950
device.  NDT_HIP_LIB selects the library to record from.  Run from the repo root:
    python tests/golden/make_chain_head_golden.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import chain_head_cases as cc            # noqa: E402


def main():
    import torch
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "chain_head.npz")
    world = cc.make_world()
    dev = (torch.from_numpy(world["sx"]).cuda(), torch.from_numpy(world["sy"]).cuda())
    torch.cuda.synchronize()
    out = {}
    for case in cc.CASES:
        got = cc.run_case(world, dev, case)
        for f in cc.FIELDS:
            out[f"{case[0]}/{f}"] = got[f]
        print(case[0], "iterations", got["iterations"].tolist(), "status", got["status"].tolist(),
              "pose", got["pose"][-1].tolist())
    np.savez_compressed(out_path, **out)
    print(f"wrote {out_path}: {len(cc.CASES)} cases, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
