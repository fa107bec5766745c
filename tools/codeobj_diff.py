#!/usr/bin/env python3
"""Compare the device code of two builds of the library, kernel by kernel.

    hipcc <HIP_FLAGS of gtsam_ndt_amd/build.py without -shared> -Iinclude --cuda-device-only -S \
          -o old.s gtsam_ndt_amd/csrc/ndt2d_api.hip        # at the parent commit; new.s at the new one
    python tools/codeobj_diff.py old.s new.s [--show]

Per kernel symbol: the instruction text (comments and .loc / .file / .cfi / .p2align / .section directives removed;
local labels lose their function number, .LBB12_3 -> .LBB_3, so that a kernel's text does not depend on its position
in the file) and the .amdhsa_* block.  Instructions are the lines that are neither labels nor directives (s_nop
included).  Prints the kernels that differ with their VGPR / SGPR / scratch / LDS numbers and instruction counts on both
sides (--show: a unified diff of each).  Exit status 0: same set of symbols, every kernel identical or with equal
resources and no more instructions than before; 1 otherwise.
"""
import difflib
import re
import sys

RES = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size", "accum_offset")


def kernels(path):
    """symbol -> (instruction lines, {amdhsa key: value})"""
    text, hsa, cur, blk = {}, {}, None, None
    types = set()
    for raw in open(path):
        line = raw.split(";", 1)[0].rstrip()
        s = line.strip()
        if not s:
            continue
        m = re.match(r"\.type\s+(\S+),@function", s)
        if m:
            types.add(m.group(1))
            continue
        if s.startswith(".amdhsa_kernel "):
            blk = s.split()[1]
            hsa[blk] = {}
            continue
        if s == ".end_amdhsa_kernel":
            blk = None
            continue
        if blk is not None:
            k, _, v = s.partition(" ")
            hsa[blk][k.replace(".amdhsa_", "")] = v.strip()
            continue
        if cur is None:
            if s.endswith(":") and s[:-1] in types:
                cur = s[:-1]
                text[cur] = []
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if re.match(r"\.(loc|file|cfi_\w+|p2align|section|text)\b", s):
            continue
        text[cur].append(re.sub(r"\.L(BB|tmp|func_\w+?)\d+", r".L\1", s))
    return {k: (text[k], hsa[k]) for k in hsa if k in text}


def n_instr(lines):
    return sum(1 for l in lines if not l.endswith(":") and not l.startswith("."))


def main():
    show = "--show" in sys.argv
    a_path, b_path = [x for x in sys.argv[1:] if not x.startswith("--")]
    a, b = kernels(a_path), kernels(b_path)
    bad = 0
    for sym in sorted(set(a) ^ set(b)):
        print(f"only in {'old' if sym in a else 'new'}: {sym}")
        bad += 1
    same = 0
    for sym in sorted(set(a) & set(b)):
        (ta, ha), (tb, hb) = a[sym], b[sym]
        if ta == tb and ha == hb:
            same += 1
            continue
        ra, rb = [ha.get(k) for k in RES], [hb.get(k) for k in RES]
        na, nb = n_instr(ta), n_instr(tb)
        ok = ra == rb and nb <= na
        bad += not ok
        nd = sum(1 for l in difflib.unified_diff(ta, tb, lineterm="", n=0)
                 if l[:1] in "+-" and l[:3] not in ("+++", "---"))
        res = " ".join(f"{k}={x}" if x == y else f"{k}={x}->{y}" for k, x, y in zip(RES, ra, rb))
        print(f"{'differs' if ok else 'CHANGED'}: {sym}\n   {res} instructions={na}->{nb} changed_lines={nd}")
        if show:
            print("\n".join(difflib.unified_diff(ta, tb, "old", "new", lineterm="", n=1)))
    print(f"{len(a)} kernels old, {len(b)} new, {same} identical, {len(set(a) & set(b)) - same} differ, "
          f"{bad} failing the bar")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
