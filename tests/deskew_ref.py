"""Independent reference for the sweep de-skewing (docs/ALGORITHM.md section 2.23): the generic matrix exponential of
u xi^ in numpy float64 - a Taylor series with scaling and squaring, nothing of the closed forms (Rodrigues, V(a)) that
the device and gtsam_ndt_amd/deskew.py use - and the moving-sensor sweeps the end-to-end tests align.  CPU only."""
import math

import numpy as np

from gtsam_ndt_amd import synth, synth3d

MOTION2 = (0.25, 0.05, 0.08)
MOTION3 = (0.5, 0.1, 0.02, 0.01, -0.01, 0.12)


def expm(A):
    """exp of a batch of square matrices [n, d, d]: scaled until every norm is below 1/2, 20 Taylor terms, squared back."""
    A = np.asarray(A, dtype=np.float64)
    norm = float(np.abs(A).sum(axis=-1).max()) if A.size else 0.0
    s = max(0, int(math.ceil(math.log2(norm / 0.5)))) if norm > 0.5 else 0
    X = A / (2.0 ** s)
    E = np.broadcast_to(np.eye(A.shape[-1]), A.shape).copy()
    term = E.copy()
    for k in range(1, 21):
        term = term @ X / k
        E = E + term
    for _ in range(s):
        E = E @ E
    return E


def hat(xi):
    """xi^ of a twist (vx, vy, omega) -> 3x3, (rho, phi) -> 4x4."""
    xi = [float(v) for v in xi]
    if len(xi) == 3:
        return np.array([[0.0, -xi[2], xi[0]], [xi[2], 0.0, xi[1]], [0.0, 0.0, 0.0]])
    r, p = xi[:3], xi[3:]
    return np.array([[0.0, -p[2], p[1], r[0]], [p[2], 0.0, -p[0], r[1]], [-p[1], p[0], 0.0, r[2]], [0.0, 0.0, 0.0, 0.0]])


def pose_matrix(pose):
    """T of a pose (x, y, theta) -> 3x3, (tx, ty, tz, roll, pitch, yaw) -> 4x4 (R = Rz Ry Rx, synth3d.rotation)."""
    pose = [float(v) for v in pose]
    if len(pose) == 3:
        T = np.eye(3)
        T[:2, :2] = synth3d.rotation(0.0, 0.0, pose[2])[:2, :2]
        T[:2, 2] = pose[:2]
        return T
    T = np.eye(4)
    T[:3, :3] = synth3d.rotation(*pose[3:])
    T[:3, 3] = pose[:3]
    return T


def euler_of(R):
    """(roll, pitch, yaw) of R = Rz Ry Rx away from gimbal lock."""
    return (math.atan2(R[2, 1], R[2, 2]), math.asin(-R[2, 0]), math.atan2(R[1, 0], R[0, 0]))


def rotation_about(axis, angle):
    """The rotation by `angle` about `axis`, by the matrix exponential."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a) * angle
    return expm(hat((0.0, 0.0, 0.0, *a))[None])[0][:3, :3]


def transform(xi, u, pts):
    """Exp(u[i] xi) pts[i] through expm: pts [n, 2] or [n, 3] float64."""
    pts = np.asarray(pts, dtype=np.float64)
    u = np.asarray(u, dtype=np.float64)
    E = expm(u[:, None, None] * hat(xi)[None])
    d = pts.shape[1]
    return np.einsum("nij,nj->ni", E[:, :d, :d], pts) + E[:, :d, d]


def ulp32(x):
    """The spacing of float32 at |x| (float64 array in, float64 out)."""
    a = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(a, np.float32(np.inf)) - a).astype(np.float64)


def bound(ref, pts, delta, rounded=True):
    """The issue's bound per coordinate: 1e-11 (|p| + |t(delta)| + 1), plus half a float32 ulp of the reference where
    the result was rounded to float32."""
    t = np.linalg.norm(np.asarray(delta[:len(delta) // 2 if len(delta) == 6 else 2], dtype=np.float64))
    b = 1e-11 * (np.linalg.norm(pts, axis=1) + t + 1.0)[:, None]
    return b + 0.5 * ulp32(ref) if rounded else b


def cast2d(sc, px, py, ang, seed, sigma_r=0.01, max_range=30.0):
    """synth.lidar_scan2d with an origin and a world bearing per beam (a sensor that moves while it sweeps): nearest
    segment hit, lidar_scan2d's noise stream, +inf where nothing is hit.  float32 ranges."""
    n = ang.size
    dx, dy = np.cos(ang)[:, None], np.sin(ang)[:, None]
    ex, ey = (sc.bx - sc.ax)[None, :], (sc.by - sc.ay)[None, :]
    wx, wy = sc.ax[None, :] - px[:, None], sc.ay[None, :] - py[:, None]
    den = dx * ey - dy * ex
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (wx * ey - wy * ex) / den
        u = (wx * dy - wy * dx) / den
    hit = (np.abs(den) > 1e-12) & (t > 1e-6) & (u >= 0.0) & (u <= 1.0)
    r = np.where(hit, t, np.inf).min(axis=1)
    i = np.arange(n, dtype=np.uint64) * np.uint64(8)
    noise = ((synth.uniform01(seed, i) + synth.uniform01(seed, i + np.uint64(1)))
             + (synth.uniform01(seed, i + np.uint64(2)) + synth.uniform01(seed, i + np.uint64(3))) - 2.0) * (math.sqrt(3.0) * sigma_r)
    return np.where(r <= max_range, r + noise, np.inf).astype(np.float32)


def matrix_pose(T):
    if T.shape[0] == 3:
        return (float(T[0, 2]), float(T[1, 2]), math.atan2(T[1, 0], T[0, 0]))
    return (float(T[0, 3]), float(T[1, 3]), float(T[2, 3]), *euler_of(T[:3, :3]))


def _scan_pose(T):
    """synth3d.lidar_scan's `pose` argument for a SENSOR frame T (4x4, map frame): lidar_scan lifts it by SENSOR_Z."""
    p = matrix_pose(T)
    return (p[0], p[1], p[2] - synth3d.SENSOR_Z, *p[3:])


def sweep3d(start, xi, n_elev, n_azim, seed=7):
    """The range image [n_elev, n_azim] of a sweep whose azimuth column j is cast from the sensor frame
    start o Exp((j / n_azim) xi) (synth3d.lidar_scan, column by column; `start` is the sensor frame in the frame of a
    static scan taken at the zero pose), and the sensor frame at the end of the sweep in that same frame.
    Returns (ranges float32, elevations, azimuth0, azimuth_inc, end_pose)."""
    lift = np.eye(4)
    lift[2, 3] = synth3d.SENSOR_Z
    A = lift @ pose_matrix(start)
    E = expm((np.arange(n_azim) / n_azim)[:, None, None] * hat(xi)[None])
    rng = np.empty((n_elev, n_azim), dtype=np.float32)
    for j in range(n_azim):
        p = synth3d.lidar_scan(seed, _scan_pose(A @ E[j]), n_elev=n_elev, n_azim=n_azim)
        rng[:, j] = np.linalg.norm(p.reshape(n_elev, n_azim, 3)[:, j], axis=1)
    el = np.deg2rad(np.linspace(-24.0, 20.0, n_elev))
    inc = 2.0 * np.pi / n_azim
    end = np.linalg.solve(lift, A @ expm(hat(xi)[None])[0])
    return rng, el, 0.5 * inc, inc, matrix_pose(end)


def sweep2d(sc, start, xi, n, seed=7):
    """The ranges of an n-beam sweep (beam i at bearing -pi + i 2 pi / n, cast from start o Exp((i / n) xi)), and the
    sensor's pose at the end of the sweep.  Returns (ranges, angle_min, angle_inc, end_pose)."""
    A = pose_matrix(start)
    E = expm((np.arange(n) / n)[:, None, None] * hat(xi)[None])
    T = A[None] @ E
    inc = 2.0 * math.pi / n
    beam = -math.pi + inc * np.arange(n)
    th = np.arctan2(T[:, 1, 0], T[:, 0, 0])
    r = cast2d(sc, T[:, 0, 2], T[:, 1, 2], th + beam, seed)
    return r, -math.pi, inc, matrix_pose(A @ expm(hat(xi)[None])[0])
