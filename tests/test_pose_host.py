"""The source-side pose rule (gtsam_ndt_amd/csrc/ndt_pose.hpp: the wrap of an angle, the nine products of R = Rz Ry Rx
and of dR/dpitch) on the CPU in its host form: the functions every kernel and host site calls, in a stand-alone program
under gcc's AddressSanitizer and UndefinedBehaviorSanitizer, held to equality of float64 bits with the Python statements
(tests/seam_ref.py rot3d_products / rot3d_pitch_products, oracle.ndt2d.wrap_angle).  The inputs of the products are the
sines and cosines themselves, so no libm enters; IEEE arithmetic rounded per operation is the same in C++ and in Python.

Which assertion catches which mutant (each is evaluated in Python on the test's own inputs and must differ somewhere):

    mutant                                   caught by
    sign_01   R[0][1] = cg sb sa + sg ca      test_products_equal_the_python_statement (every input with sg ca != 0)
    open_at_minus_pi   t < -pi for t <= -pi   test_wrap_angle_equals_the_oracle (the input -pi: +pi is expected)
"""
import math
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import seam_cases as SC
import seam_ref as S
import tilted_cases as TC
from oracle import ndt2d as o2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PI = math.pi
N_RANDOM = 20000


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("san") / "pose")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "gtsam_ndt_amd", "csrc"),
           os.path.join(ROOT, "tests", "cpp", "pose_main.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT)
    return exe


def _run(driver, lines):
    p = subprocess.run([driver], input="".join(lines), capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    out = p.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def _bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


# ------------------------------------------------------------------------------------------------ the products
def _angle_triples():
    """(roll, pitch, yaw): the attitudes of tilted_cases, the 3D poses of seam_cases, pitch next to +-pi/2, roll at +-pi,
    and seeded random triples."""
    tri = [tuple(a) for a in TC.ATTITUDES.values()] + [tuple(TC.SINGULAR)]
    tri += [tuple(p[3:6]) for p in SC.POSES_3D.values()]
    for sign in (1.0, -1.0):
        for d in (0.0, 1e-9, -1e-9, 1e-12, -1e-12):
            tri.append((0.4, sign * (PI / 2.0 + d), -0.3))
            tri.append((-2.0, sign * (PI / 2.0 + d), 2.9))
        tri += [(sign * PI, 0.3, 0.7), (sign * PI, -1.2, -2.5), (sign * PI, sign * PI / 2.0, sign * PI)]
    rng = np.random.default_rng(20240607)
    tri += [tuple(t) for t in rng.uniform(-PI, PI, size=(N_RANDOM, 3))]
    return tri


def _sincos(tri):
    a, b, g = (float(v) for v in tri)
    return (math.sin(a), math.cos(a), math.sin(b), math.cos(b), math.sin(g), math.cos(g))


def _sign_01(sa, ca, sb, cb, sg, cg):
    e = S.rot3d_products(sa, ca, sb, cb, sg, cg)
    e[1] = cg * sb * sa + sg * ca
    return e


def test_products_equal_the_python_statement(driver):
    sc = [_sincos(t) for t in _angle_triples()]
    assert len(sc) >= N_RANDOM + 30
    out = _run(driver, ["R " + " ".join(str(_bits(v)) for v in six) + "\n" for six in sc])
    mutant_differs = 0
    for six, line in zip(sc, out):
        got = [int(v) for v in line.split()]
        want = S.rot3d_products(*six) + S.rot3d_pitch_products(*six)
        assert got == [_bits(v) for v in want], (six, line)
        mutant_differs += [_bits(v) for v in _sign_01(*six)] != got[:9]
    assert mutant_differs > N_RANDOM // 2                      # sign_01 would have been caught


def test_products_are_those_of_the_pose_mirrors():
    """The plumbing round the one statement, not evidence that three statements agree: all three mirrors call
    rot3d_products, so this pins only which sines and cosines each hands it (rot3d_entries and point_fit_ref.rotation32
    wrap the angles first, map_merge_ref.rotation does not, as the host's merge_rotation does not), the float32 step of
    rotation32 and the row-major reshape.  That the mirrors' former own texts gave the same bits was shown once, when
    they were replaced (0 differences on the poses their users pass), and cannot be run again."""
    import map_merge_ref as M
    import point_fit_ref as F
    for p in SC.POSES_3D.values():
        a, b, g = (o2.wrap_angle(float(v)) for v in p[3:6])
        want = S.rot3d_products(math.sin(a), math.cos(a), math.sin(b), math.cos(b), math.sin(g), math.cos(g))
        assert S.rot3d_entries(*p[3:6]) == want
        assert F.rotation32(p, 3)[0].ravel().tolist() == [float(np.float32(v)) for v in want]
        Rm, t = M.rotation(3, p)                               # (the host does not wrap)
        assert Rm[0] + Rm[1] + Rm[2] == S.rot3d_products(*_sincos(p[3:6])) and t == list(p[:3])


# ------------------------------------------------------------------------------------------------ the wrap
def _wrap_inputs():
    v = [0.0, -0.0, PI, -PI, 3.0 * PI, -3.0 * PI, 1e6, -1e6, 1e15, -1e15]
    for x in (PI, -PI):
        v += [math.nextafter(x, math.inf), math.nextafter(x, -math.inf)]
    v += [float(p[2]) for p in SC.POSES_2D.values()]
    v += [float(x) for x in np.random.default_rng(20240608).uniform(-50.0, 50.0, size=N_RANDOM)]
    return v


def _open_at_minus_pi(t):
    if t > PI or t < -PI:
        t = t - 2.0 * PI * math.floor((t + PI) / (2.0 * PI))
        if t < -PI:
            t += 2.0 * PI
    return t


def test_wrap_angle_equals_the_oracle(driver):
    v = _wrap_inputs()
    out = _run(driver, [f"W {_bits(x)}\n" for x in v])
    mutant_differs = 0
    for x, line in zip(v, out):
        want = o2.wrap_angle(x)
        assert -PI < want <= PI
        assert int(line) == _bits(want), (x, line)
        mutant_differs += _bits(_open_at_minus_pi(x)) != int(line)
    assert int(out[v.index(-PI)]) == _bits(PI)                 # -pi itself goes to +pi
    assert mutant_differs > 0                                  # open_at_minus_pi would have been caught
