"""The exact reference of the cell lookup (docs/ALGORITHM.md 2.1, 2.4, 2.6, 2.19): which cell a source point belongs
to, restated so that there is exactly one right answer per point - also for a point that lies on a cell seam or one
ulp off it, where every other reference of the suite looks away.

- fma32: a correctly rounded float32 fma.  The float64 product of two float32 values is exact; the float64 sum may be
  rounded, and rounding that sum to float32 again is wrong only where the rounded sum sits exactly on a float32 tie.
  Those cases are settled by the exact error term of the float64 sum (two-sum); fma32_fraction is the same operation in
  rationals, the definition tests/test_seam_ref.py holds fma32 to.
- image2d / image3d / image3d_batch: the image recipes of the kernel families, operation by operation.
- rot2d32 / rot3d32: cs, sn and the nine R entries as float32(float64 value), and tie_margin: how far (in float64
  ulps) such a value is from a float32 rounding tie.  The device's sine and cosine are within 1 ulp of the float64
  value, so a pose whose values all keep a margin rounds to the same float32 numbers there.  A condition on the inputs.
- keys2d / keys3d: the float32 key rules (oracle.ndt2d.cell_keys32, oracle.ndt3d.cell_keys3).
- seam: the smallest float32 x whose cell index reaches k, found on the rule itself.
"""
import math
from fractions import Fraction

import numpy as np

from oracle import ndt2d as o2
from oracle import ndt3d as o3

F32 = np.float32
CLAMP = F32(1e15)          # image_point: coordinates are clamped to +-1e15 (v_med3_f32) before the chain


# ------------------------------------------------------------------------------------------------ exact float32 fma
def round_fraction32(v: Fraction) -> np.float32:
    """The rational v rounded to the nearest float32, ties to even (finite results only)."""
    r = F32(float(v))                                     # at most one float32 away from the right answer
    cand = [np.nextafter(r, F32(-np.inf)), r, np.nextafter(r, F32(np.inf))]
    cand = [c for c in cand if np.isfinite(c)]
    dist = [abs(Fraction(float(c)) - v) for c in cand]
    best = min(dist)
    pick = [c for c, d in zip(cand, dist) if d == best]
    if len(pick) == 2:                                    # a true tie: the even mantissa
        pick = [c for c in pick if (int(np.array(c, F32).view(np.uint32)) & 1) == 0]
    return F32(pick[0])


def fma32_fraction(a, b, c) -> np.float32:
    """fma(a, b, c) of three finite float32 scalars in rationals: the definition fma32 is held to."""
    return round_fraction32(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


fma32 = o2.fma32          # the correctly rounded float32 fma (two-sum on the float64 sum), shared with the oracle's mirror


def fma32_double_rounded(a, b, c):
    """The emulation the suite used before: float64 multiply-add rounded to float32 (wrong on the ties above)."""
    return (np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64)
            + np.asarray(c, F32).astype(np.float64)).astype(F32)


# ------------------------------------------------------------------------------------------------ rotations, tie margin
def tie_margin(v: float) -> float:
    """Distance of the float64 v from the nearest float32 rounding tie, in float64 ulps of v (inf for v = 0)."""
    v = float(v)
    if v == 0.0:
        return math.inf
    r = F32(v)
    lo, hi = np.nextafter(r, F32(-np.inf)), np.nextafter(r, F32(np.inf))
    d = min(abs(v - 0.5 * (float(lo) + float(r))), abs(v - 0.5 * (float(r) + float(hi))))
    return d / float(np.spacing(abs(v)))


def rot2d32(theta: float):
    """(cs, sn) float32 of the wrapped angle, and the float64 values they were rounded from."""
    th = o2.wrap_angle(float(theta))
    c, s = math.cos(th), math.sin(th)
    return F32(c), F32(s), (c, s)


def rot3d_products(sa, ca, sb, cb, sg, cg):
    """rot3_products of csrc/ndt_pose.hpp in its host form: the nine float64 products of R = Rz Ry Rx, row-major, from the
    sines and cosines of roll (a), pitch (b) and yaw (g), every operation rounded separately.  The one Python statement:
    map_merge_ref.rotation and point_fit_ref.rotation32 call it, tests/test_pose_host.py holds the C++ to it bit for bit."""
    return [cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa,
            sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa,
            -sb, cb * sa, cb * ca]


def rot3d_pitch_products(sa, ca, sb, cb, sg, cg):
    """rot3_pitch_products of csrc/ndt_pose.hpp in its host form: dR/dpitch = Rz dRy Rx, row-major."""
    return [-cg * sb, cg * cb * sa, cg * cb * ca,
            -sg * sb, sg * cb * sa, sg * cb * ca,
            -cb, -sb * sa, -sb * ca]


def rot3d_entries(roll: float, pitch: float, yaw: float):
    """The nine float64 products of the kernels' R (make_rt3, make_rot3; csrc/ndt3d_kernels.hpp) at the wrapped angles."""
    a, b, g = (o2.wrap_angle(float(v)) for v in (roll, pitch, yaw))
    return rot3d_products(math.sin(a), math.cos(a), math.sin(b), math.cos(b), math.sin(g), math.cos(g))


def rot3d32(roll, pitch, yaw):
    e = rot3d_entries(roll, pitch, yaw)
    return np.array(e, np.float64).astype(F32), e


def pose_margin(pose, dim: int):
    """(worst margin over the pose's rotation values in float64 ulps, the slack in ulps the pose must keep).
    Slack: 4 ulps (the issue's figure: the device's sincos is within 1).  A 2D angle outside (-pi, pi] is wrapped first,
    one more float64 rounding of up to half an ulp of the angle; the 3D entries are sums of products of sines and cosines
    that a compiler may contract: both move a value by a few 1e-16 absolute, so such poses must keep 1e-14 absolute."""
    if dim == 2:
        _, _, vals = rot2d32(pose[2])
        absolute = 0.0 if -math.pi < float(pose[2]) <= math.pi else 1e-14
    else:
        vals = rot3d_entries(*pose[3:6])
        single_axis = float(pose[3]) == 0.0 and float(pose[4]) == 0.0 and -math.pi < float(pose[5]) <= math.pi
        absolute = 0.0 if single_axis else 1e-14
    worst, need = math.inf, 4.0
    for v in vals:
        if v == 0.0:
            continue
        need_v = 4.0 + absolute / float(np.spacing(abs(v)))
        m = tie_margin(v)
        if m - need_v < worst - need:
            worst, need = m, need_v
    return worst, need


def pose_is_tie_free(pose, dim: int) -> bool:
    worst, need = pose_margin(pose, dim)
    return worst > need


# ------------------------------------------------------------------------------------------------ image recipes
def _clamped(v):
    """v_med3_f32(v, -1e15, 1e15); a NaN gives a finite bound (which one does not matter: both are far outside)."""
    v = np.asarray(v, F32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(v), -CLAMP, np.clip(v, -CLAMP, CLAMP)).astype(F32)


def image2d(x, y, pose, fma=fma32):
    """ALGORITHM 2.4 / image_point: p' = (fma(cs, x, fma(-sn, y, tx)), fma(sn, x, fma(cs, y, ty)))."""
    cs, sn, _ = rot2d32(pose[2])
    tx, ty = F32(pose[0]), F32(pose[1])
    x, y = _clamped(x), _clamped(y)
    return fma(cs, x, fma(-sn, y, tx)), fma(sn, x, fma(cs, y, ty))


def image2d_float64(x, y, pose):
    """The mutant: the image in float64, rounded once."""
    th = o2.wrap_angle(float(pose[2]))
    c, s = math.cos(th), math.sin(th)
    x, y = _clamped(x).astype(np.float64), _clamped(y).astype(np.float64)
    return (c * x - s * y + float(pose[0])).astype(F32), (s * x + c * y + float(pose[1])).astype(F32)


def image3d(x, y, z, pose, fma=fma32):
    """ALGORITHM 2.6 / image_row3: p'_r = fma(R_r0, x, fma(R_r1, y, fma(R_r2, z, t_r))): every kernel but k_batch3."""
    R, _ = rot3d32(*pose[3:6])
    x, y, z = _clamped(x), _clamped(y), _clamped(z)
    return tuple(fma(R[3 * r], x, fma(R[3 * r + 1], y, fma(R[3 * r + 2], z, F32(pose[r])))) for r in range(3))


def image3d_batch(x, y, z, pose, fma=fma32):
    """k_batch3 (csrc/ndt3d_batch.hpp, consume_set): y_r = fma(R_r0, x, fma(R_r1, y, R_r2 * z)), then p'_r = y_r + t_r:
    one rounding more than the chain, so a point within an ulp of a seam may lie in the other voxel."""
    R, _ = rot3d32(*pose[3:6])
    x, y, z = _clamped(x), _clamped(y), _clamped(z)
    out = []
    for r in range(3):
        yr = fma(R[3 * r], x, fma(R[3 * r + 1], y, (R[3 * r + 2] * z).astype(F32)))
        out.append((yr + F32(pose[r])).astype(F32))
    return tuple(out)


def image3d_float64(x, y, z, pose):
    R = np.array(rot3d_entries(*pose[3:6])).reshape(3, 3)
    P = np.stack([_clamped(x), _clamped(y), _clamped(z)], axis=1).astype(np.float64)
    Pw = (P @ R.T + np.array([float(v) for v in pose[:3]])).astype(F32)
    return Pw[:, 0], Pw[:, 1], Pw[:, 2]


# ------------------------------------------------------------------------------------------------ keys
def finite_points(*coords):
    return np.all([np.isfinite(np.asarray(c, F32)) for c in coords], axis=0)


def keys2d(px, py, geom):
    """geom = (ox, oy, inv_c, W, H).  (key, inside): floorf((p' - o) * inv_c) in float32, 0 <= f < extent.  The device
    clamps the index onto the grid instead; the ring holds no valid cell, so `inside & valid[key]` is what it reads."""
    return o2.cell_keys32(np.asarray(px, F32), np.asarray(py, F32), *geom)


def keys3d(px, py, pz, geom):
    """geom = (o [3] float32, inv_c, dims)."""
    o, inv_c, dims = geom
    P = np.stack([np.asarray(px, F32), np.asarray(py, F32), np.asarray(pz, F32)], axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((P - np.asarray(o, F32)) * F32(inv_c))
    inside = np.all((f >= 0) & (f < np.array(dims, np.float32)), axis=1)
    idx = np.where(inside[:, None], f, 0).astype(np.int64)
    key = (idx[:, 2] * dims[1] + idx[:, 1]) * dims[0] + idx[:, 0]
    return key, inside, idx


def cell_index32(x, o, inv_c):
    """floorf((x - o) * inv_c), float32 operations, as float64 integers (may be huge or non-finite)."""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.floor((np.asarray(x, F32) - F32(o)) * F32(inv_c)).astype(np.float64)


def seam(o, inv_c, k: int) -> np.float32:
    """The smallest float32 x with floorf((x - o) * inv_c) >= k: found by stepping on the rule, not taken as o + k c."""
    o, inv_c = F32(o), F32(inv_c)
    # the rule is monotone in x, so the seam is found by bisection over the float32 values in their order (next to 0 the
    # values are too dense to walk: the seam of o = -0.1 next to x = 0 is about -3.7e-9, 2^90 steps below 0), and the two
    # values either side of it are then checked on the rule itself
    span = 4.0 * (abs(float(o)) + (abs(k) + 2) / float(inv_c)) + 1.0
    lo, hi = _ordinal(F32(-span)), _ordinal(F32(span))
    assert cell_index32(_from_ordinal(lo), o, inv_c) < k <= cell_index32(_from_ordinal(hi), o, inv_c)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if cell_index32(_from_ordinal(mid), o, inv_c) >= k:
            hi = mid
        else:
            lo = mid
    x = _from_ordinal(hi)
    assert cell_index32(x, o, inv_c) >= k > cell_index32(np.nextafter(x, F32(-np.inf)), o, inv_c)
    return x


def _ordinal(x) -> int:
    """The position of a finite float32 in the order of all float32 values (-0.0 and +0.0 share 0)."""
    b = int(np.array(x, F32).view(np.int32))
    return b if b >= 0 else -(b & 0x7FFFFFFF)


def _from_ordinal(n: int) -> np.float32:
    return np.array(n if n >= 0 else (-n) | 0x80000000, np.uint32).view(F32)[()]


def below(x) -> np.float32:
    return np.nextafter(F32(x), F32(-np.inf))


def above(x) -> np.float32:
    return np.nextafter(F32(x), F32(np.inf))


# the mutants of the key rule (tests/test_seam_ref.py): each must change the expected hits of a named catalogue entry
def index_mutant(name: str, x, o, inv_c, c: float, extent: int):
    """(index, inside) per coordinate under a mutated rule; "rule" is the stated one."""
    x = np.asarray(x, F32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if name == "divide":                                   # (x - o) / c instead of (x - o) * inv_c
            f = (x - F32(o)) / F32(c)
        else:
            f = (x - F32(o)) * F32(inv_c)
        if name == "truncate":                                 # (int)f without the floor: (-1, 0) becomes cell 0
            i = np.trunc(f)
            inside = (f > -1) & (i < extent)
        elif name == "upper_inclusive":                        # f <= extent
            i = np.minimum(np.floor(f), extent - 1)
            inside = (f >= 0) & (f <= extent)
        else:
            i = np.floor(f)
            inside = (i >= 0) & (i < extent)
    return np.where(inside, i, 0).astype(np.int64), inside
