"""The call record of the C++ adapter (include/ndt_matcher_hip.hpp): tests/cpp/adapter_calls_main.cpp calls every public
member once per dimension against the recording stand-in for the library, tests/cpp/adapter_stub.cpp; this module builds
that program under gcc's AddressSanitizer and UndefinedBehaviorSanitizer (a stand-alone program), runs it once per test
session and parses what it printed.  Needs neither a device nor the built library."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "adapter_calls.txt")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
MODES = ("ok", "fail", "fail-after-wait")


def build_and_run(include_dir, work_dir):
    """The record (the program's standard output) with the adapter found in include_dir."""
    exe = os.path.join(work_dir, "adapter_calls")
    cmd = ["g++", *FLAGS, "-I", include_dir, os.path.join(ROOT, "tests", "cpp", "adapter_stub.cpp"),
           os.path.join(ROOT, "tests", "cpp", "adapter_calls_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0 and "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-3000:]
    return p.stdout


@functools.lru_cache(maxsize=None)
def record():
    """The record of the header in this tree, built and run once per session."""
    work = tempfile.mkdtemp(prefix="adapter_calls_")
    atexit.register(shutil.rmtree, work, ignore_errors=True)
    return build_and_run(os.path.join(ROOT, "include"), work)


def parse(text):
    """{(section, mode): [C function, ...]} in the order of the calls; a section is "Class.method" or a free function's
    name, with "/case" behind it where an edge has a section of its own."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.fullmatch(r"== (\S+) \[([a-z-]+)\]", line)
        if m:
            cur = out.setdefault((m.group(1), m.group(2)), [])
            assert m.group(2) in MODES, line
        elif line.startswith("  C "):
            cur.append(line.split()[1])
    return out


@functools.lru_cache(maxsize=None)
def calls():
    """{"Class.method": [C functions the method called while every call succeeded]}, its "/case" sections included."""
    out = {}
    for (name, mode), fns in parse(record()).items():
        if mode == "ok":
            out.setdefault(name.split("/")[0], []).extend(fns)
    return out


def called_by(method):
    """The C functions that NdtMatcherHip.method and NdtMatcherHip3.method call: (2D list, 3D list)."""
    c = calls()
    return c["NdtMatcherHip." + method], c["NdtMatcherHip3." + method]


def both_call(method, fn):
    """Whether NdtMatcherHip.method calls ndt2d_<fn> and NdtMatcherHip3.method calls ndt3d_<fn>."""
    c2, c3 = called_by(method)
    return "ndt2d_" + fn in c2 and "ndt3d_" + fn in c3


def statuses(text):
    """{C function: {mode: set of statuses it returned in sections of that mode}}, for the entry points that return one."""
    out, mode = {}, None
    for line in text.splitlines():
        m = re.fullmatch(r"== (\S+) \[([a-z-]+)\]", line)
        if m:
            mode = m.group(2)
            continue
        m = re.fullmatch(r"  C (\S+) .* -> (-?\d+)", line)
        if m:
            out.setdefault(m.group(1), {}).setdefault(mode, set()).add(int(m.group(2)))
    return out


def all_called():
    """Every C function some adapter method calls."""
    return {fn for fns in calls().values() for fn in fns}
