#!/usr/bin/env python3
"""Generates tests/golden/cell_records.npz: the exact per-cell records (valid cells' keys, mean, clamped Sigma^-1,
clamped Sigma, kappa) of every catalogue of tests/cell_record_cases.py under every (min_points, eig_ratio) pair of its
PARAMS, by tests/cell_record_ref.py exact_cells - integers, fractions and mpmath at 60 digits.  The GPU tests read the
file because a GPU machine may have no mpmath; tests/test_cell_record_ref.py regenerates it and compares.  No device is
needed.  Run from the repo root:
    python tests/golden/make_cell_records_golden.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cell_record_cases as K            # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else K.GOLDEN
    out = K.golden_arrays()
    np.savez_compressed(out_path, **out)
    cells = sum(v.size for k, v in out.items() if k.endswith("/key"))
    print(f"wrote {out_path}: {cells} valid cells over {len(K.PARAMS)} parameter sets, {os.path.getsize(out_path)} bytes")


if __name__ == "__main__":
    main()
