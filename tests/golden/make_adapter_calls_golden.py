#!/usr/bin/env python3
"""Generates tests/golden/adapter_calls.txt: what tests/cpp/adapter_calls_main.cpp prints against the recording stand-in
tests/cpp/adapter_stub.cpp - every C call of every public member of include/ndt_matcher_hip.hpp with its arguments, and
every field of what the member returned.

The fixture pins the adapter across changes that may only restate it, so it is recorded with the header as it was BEFORE
such a change, never from the header under test.  The committed file was written by this script from the header of commit
65ed764 ("State the 3D rotation products and the search kernels' task once each"), in which NdtMatcherHip and
NdtMatcherHip3 were still two classes written out in full, the parent of the commit that built both on one core.  Needs
g++ and git, no device.  Run from the repo root:
    python tests/golden/make_adapter_calls_golden.py [revision] [out.txt]
"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adapter_calls as AC            # noqa: E402


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else "65ed764"
    out_path = sys.argv[2] if len(sys.argv) > 2 else AC.GOLDEN
    work = tempfile.mkdtemp(prefix="adapter_golden_")
    try:
        inc = os.path.join(work, "include")
        os.mkdir(inc)
        for name in ("ndt_matcher_hip.hpp", "ndt_hip.h"):
            with open(os.path.join(inc, name), "wb") as f:
                f.write(subprocess.run(["git", "show", f"{rev}:include/{name}"], check=True, cwd=ROOT, capture_output=True).stdout)
        text = AC.build_and_run(inc, work)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    with open(out_path, "w") as f:
        f.write(text)
    print(f"wrote {out_path} from {rev}: {len(AC.parse(text))} sections, {text.count(chr(10))} lines, {len(text)} bytes")


if __name__ == "__main__":
    main()
