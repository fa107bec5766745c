"""Host restatement of the sweep de-skewing (docs/ALGORITHM.md section 2.23) in numpy float64, closed form - what the
device entry points ndt2d/ndt3d_*_deskew_dev and ndt2d/ndt3d_deskew_points_dev compute, for a caller without a device
and for tests.  Results are float64: round with .astype(np.float32) to compare with the device.

`delta` is the sensor's pose at the end of the sweep in the sensor frame at its start: (dx, dy, dtheta) or
(tx, ty, tz, roll, pitch, yaw) with R = Rz Ry Rx.  The motion within the sweep is the constant twist xi = Log(delta); a
point p measured at sweep fraction s becomes Exp((s - ref_frac) xi) p, in the sensor frame at fraction ref_frac.
"""
from __future__ import annotations

import math

import numpy as np

SMALL_ANGLE = 1e-4        # below it sin a / a and its kin come from their power series
MAX_ANGLE_3D = 3.1        # a 3D delta that turns by this much or more is refused


def _wrap(t: float) -> float:
    if t > math.pi or t <= -math.pi:
        t = t - 2.0 * math.pi * math.floor((t + math.pi) / (2.0 * math.pi))
        if t <= -math.pi:
            t += 2.0 * math.pi
    return t


def _rotation(roll, pitch, yaw):
    ca, sa, cb, sb, cg, sg = math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch), math.cos(yaw), math.sin(yaw)
    return np.array([[cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa],
                     [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa],
                     [-sb, cb * sa, cb * ca]])


def _check(v, n, what):
    v = tuple(float(x) for x in v)
    if len(v) != n or not all(math.isfinite(x) for x in v):
        raise ValueError(f"{what} must be {n} finite numbers")
    return v


def sweep_motion(prev, cur):
    """prev^-1 o cur of two poses (3- or 6-vectors) in one frame: the constant-velocity guess of the motion within the
    next sweep.  cur == prev gives exact zeros."""
    n = len(prev)
    if n not in (3, 6):
        raise ValueError("a pose has 3 or 6 entries")
    prev, cur = _check(prev, n, "prev"), _check(cur, n, "cur")
    if n == 3:
        c, s = math.cos(prev[2]), math.sin(prev[2])
        dx, dy = cur[0] - prev[0], cur[1] - prev[1]
        return (c * dx + s * dy, c * dy - s * dx, _wrap(cur[2] - prev[2]))
    if prev == cur:
        return (0.0,) * 6
    Rp, Rc = _rotation(*prev[3:]), _rotation(*cur[3:])
    R = Rp.T @ Rc
    t = Rp.T @ (np.array(cur[:3]) - np.array(prev[:3]))
    pitch = math.asin(min(1.0, max(-1.0, -R[2, 0])))
    if abs(math.cos(pitch)) < 1e-12:                   # roll and yaw share an axis: roll = 0 by choice
        roll, yaw = 0.0, math.atan2(-R[0, 1], R[1, 1])
    else:
        roll, yaw = math.atan2(R[2, 1], R[2, 2]), math.atan2(R[1, 0], R[0, 0])
    return (float(t[0]), float(t[1]), float(t[2]), roll, pitch, yaw)


def motion_twist(delta):
    """xi = Log(delta): (vx, vy, omega) for a 3-vector, (rho[3], phi[3]) for a 6-vector."""
    n = len(delta)
    if n not in (3, 6):
        raise ValueError("a motion has 3 or 6 entries")
    d = _check(delta, n, "delta")
    if n == 3:
        w = _wrap(d[2])
        h = 0.5 * w
        sh, ch = math.sin(h), math.cos(h)
        k = 1.0 - h * h / 6.0 if abs(h) < SMALL_ANGLE else sh / h            # V(w)^-1 = R(-h) / sinc(h)
        return ((ch * d[0] + sh * d[1]) / k, (ch * d[1] - sh * d[0]) / k, w)
    ca, sa, cb, sb = math.cos(0.5 * d[3]), math.sin(0.5 * d[3]), math.cos(0.5 * d[4]), math.sin(0.5 * d[4])
    cg, sg = math.cos(0.5 * d[5]), math.sin(0.5 * d[5])
    qw = cg * cb * ca + sg * sb * sa                                          # q = qz qy qx
    v = np.array([cg * cb * sa - sg * sb * ca, cg * sb * ca + sg * cb * sa, sg * cb * ca - cg * sb * sa])
    if qw < 0.0:
        qw, v = -qw, -v
    vn = math.sqrt(float(v @ v))
    half = math.atan2(vn, qw)
    theta = 2.0 * half
    if theta >= MAX_ANGLE_3D:
        raise ValueError("the sweep's rotation is 3.1 rad or more: its logarithm is ill-conditioned")
    phi = v * (2.0 + vn * vn / 3.0 if vn < SMALL_ANGLE else theta / vn)
    D = 1.0 / 12.0 + theta * theta / 720.0 if theta < SMALL_ANGLE else (1.0 - half * math.cos(half) / math.sin(half)) / (theta * theta)
    t = np.array(d[:3])
    pt = np.cross(phi, t)
    rho = t - 0.5 * pt + D * np.cross(phi, pt)
    return (*(float(x) for x in rho), *(float(x) for x in phi))


def exp_apply(xi, u, pts):
    """Exp(u[i] xi) pts[i]: xi a twist of motion_twist, u [n] float64, pts [n, 2] or [n, 3] float64."""
    xi = np.asarray(xi, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    p = np.asarray(pts, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        if xi.size == 3:
            h = 0.5 * (u * xi[2])
            sh, ch = np.sin(h), np.cos(h)
            k = u * np.where(np.abs(h) < SMALL_ANGLE, 1.0 - h * h / 6.0, sh / np.where(h == 0.0, 1.0, h))
            s, c = 2.0 * sh * ch, 1.0 - 2.0 * sh * sh
            tx, ty = k * (ch * xi[0] - sh * xi[1]), k * (sh * xi[0] + ch * xi[1])
            return np.stack([(c * p[:, 0] - s * p[:, 1]) + tx, (s * p[:, 0] + c * p[:, 1]) + ty], axis=1)
        w = u[:, None] * xi[None, 3:]
        r = u[:, None] * xi[None, :3]
        a2 = np.einsum("ij,ij->i", w, w)
        al = np.sqrt(a2)
        small = al < SMALL_ANGLE
        h = np.where(small, 1.0, 0.5 * al)
        k = np.sin(h) / h
        A = np.where(small, 1.0 - a2 / 6.0, k * np.cos(h))
        B = np.where(small, 0.5 - a2 / 24.0, 0.5 * k * k)
        Cc = np.where(small, 1.0 / 6.0 - a2 / 120.0, (1.0 - A) / np.where(small, 1.0, a2))
        wp = np.cross(w, p)
        wr = np.cross(w, r)
        A, B, Cc = A[:, None], B[:, None], Cc[:, None]
        return (p + A * wp + B * np.cross(w, wp)) + (r + B * wr + Cc * np.cross(w, wr))


def deskew_points(coords, frac, motion, ref_frac: float = 1.0):
    """coords: 2 or 3 arrays [n]; frac [n] the sweep fraction of each point.  Returns [n, dim] float64.  A point whose
    fraction equals ref_frac, and every point when motion is all zero, comes back unchanged; a point with a non-finite
    fraction comes back NaN."""
    p = np.stack([np.asarray(c, dtype=np.float64) for c in coords], axis=1)
    if len(motion) != (3 if p.shape[1] == 2 else 6):
        raise ValueError("the motion's length does not fit the points' dimension")
    if not math.isfinite(ref_frac):
        raise ValueError("ref_frac must be finite")
    xi = motion_twist(motion)
    f = np.asarray(frac, dtype=np.float64)
    u = f - float(ref_frac)
    out = p.copy()
    move = (u != 0.0) & np.isfinite(f) & bool(any(x != 0.0 for x in xi))
    out[move] = exp_apply(xi, u[move], p[move])
    out[~np.isfinite(f)] = np.nan
    return out


def _frac(frac, n):
    f0, finc = (0.0, 1.0 / n) if frac is None else (float(frac[0]), float(frac[1]))
    if not (math.isfinite(f0) and math.isfinite(finc)):
        raise ValueError("frac must be two finite numbers")
    return f0 + finc * np.arange(n, dtype=np.float64)


def polar_to_points(ranges, angle_min, angle_inc, range_min=0.0, range_max=1e30, *, motion, frac=None, ref_frac=1.0):
    """ndt2d_polar_to_points_deskew_dev on the host: [n, 2] float64, invalid returns NaN.  Beam i was fired at fraction
    frac[0] + i frac[1] (default (0, 1 / n))."""
    r32 = np.asarray(ranges, dtype=np.float32).ravel()
    r = r32.astype(np.float64)
    ang = angle_min + angle_inc * np.arange(r.size, dtype=np.float64)
    ok = np.isfinite(r32) & (r32 >= np.float32(range_min)) & (r32 <= np.float32(range_max))
    with np.errstate(invalid="ignore"):
        out = deskew_points((r * np.cos(ang), r * np.sin(ang)), _frac(frac, r.size), motion, ref_frac)
    out[~ok] = np.nan
    return out


def range_image_to_points(ranges, elevations, azimuth0, azimuth_inc, range_min=0.0, range_max=1e30, *, motion, frac=None,
                          ref_frac=1.0):
    """ndt3d_range_image_to_points_deskew_dev on the host: [n_elev * n_azim, 3] float64, ring-major.  Azimuth column j
    (every ring of it) was fired at fraction frac[0] + j frac[1] (default (0, 1 / n_azim))."""
    r32 = np.asarray(ranges, dtype=np.float32)
    n_elev, n_azim = r32.shape
    r = r32.astype(np.float64)
    el = np.asarray(elevations, dtype=np.float64)
    az = azimuth0 + azimuth_inc * np.arange(n_azim, dtype=np.float64)
    ce, se = np.cos(el)[:, None], np.sin(el)[:, None]
    ok = (np.isfinite(r32) & (r32 >= np.float32(range_min)) & (r32 <= np.float32(range_max))).ravel()
    with np.errstate(invalid="ignore"):
        x, y, z = r * (ce * np.cos(az)[None, :]), r * (ce * np.sin(az)[None, :]), r * (se * np.ones((1, n_azim)))
        f = np.broadcast_to(_frac(frac, n_azim)[None, :], (n_elev, n_azim)).ravel()
        out = deskew_points((x.ravel(), y.ravel(), z.ravel()), f, motion, ref_frac)
    out[~ok] = np.nan
    return out
