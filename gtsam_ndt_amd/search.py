"""Host restatement of the exhaustive pose searches (docs/ALGORITHM.md "Exhaustive pose search" and "Exhaustive 3D pose
search"), in the spirit of synth.scan_points: the lattice of a window and the peak / separation rules, in numpy.  It is
the specification the tests hold ndt2d_search_* and ndt3d_search_* to; nothing on the GPU path calls it.  select_best
is the same for the hits of a scored pose list (ndt2d_best_poses_dev, ndt3d_best_poses_dev).

A window is (center, half_extent, step); ``Window`` names the three.  2D: each an (x, y, theta) triple.  3D: the
centre is a 6-vector (tx, ty, tz, roll, pitch, yaw) whose indices 0, 1, 5 are searched (half_extent and step stay
(x, y, yaw) triples) and whose tz, roll, pitch are pinned; the hits then carry 6-vector poses.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

PI = 3.141592653589793
MAX_POSES = 1 << 25
SHORTLIST = 4096


class Window(NamedTuple):
    center: tuple
    half_extent: tuple
    step: tuple


@dataclass(frozen=True)
class SearchHit:
    pose: tuple        # (x, y, theta), theta wrapped to (-pi, pi]; a 3D window: (x, y, tz, roll, pitch, yaw)
    score: float       # the lattice score (a float32 value)
    index: int         # flat lattice index ((j * n_y) + iy) * n_x + ix


class CapacityError(ValueError):
    """The window holds more than 2^25 poses (NDT_ERR_CAPACITY)."""


def wrap(t):
    """The library's wrap_angle, elementwise in float64 (the same operations in the same order)."""
    t = np.asarray(t, dtype=np.float64)
    out = t.copy()
    m = (t > PI) | (t <= -PI)
    v = t[m] - 2.0 * PI * np.floor((t[m] + PI) / (2.0 * PI))
    v = np.where(v <= -PI, v + 2.0 * PI, v)
    out[m] = v
    return out


def _check(window):
    c, h, s = (tuple(float(v) for v in a) for a in window)
    if len(c) not in (3, 6) or len(h) != 3 or len(s) != 3:
        raise ValueError("center is an (x, y, theta) triple or a 6-vector pose; half_extent and step are triples")
    for v in c + h + s:
        if not math.isfinite(v):
            raise ValueError("non-finite window value")
    if len(c) == 6:
        c = (c[0], c[1], c[5])             # the searched axes of a 3D window
    if any(not v >= 0.0 for v in h) or any(not v > 0.0 for v in s):
        raise ValueError("half extents must be >= 0 and steps > 0")
    return c, h, s


def dims(window):
    """(n_theta, n_y, n_x) and whether the heading axis is cyclic (ndt2d_search_lattice_size)."""
    c, h, s = _check(window)
    n = [2.0 * math.floor(h[a] / s[a] + 1e-9) + 1.0 for a in range(3)]
    cyclic = h[2] >= PI
    if cyclic:
        n[2] = max(1.0, math.floor(2.0 * PI / s[2] + 0.5))
    if max(n) > MAX_POSES or n[0] * n[1] * n[2] > MAX_POSES:
        raise CapacityError("the search window holds more than 2^25 lattice poses")
    return (int(n[2]), int(n[1]), int(n[0])), cyclic


def lattice(window):
    """The axes of the window's lattice as float64 arrays: (x, y, theta), theta wrapped to (-pi, pi]."""
    c, h, s = _check(window)
    (nt, ny, nx), cyclic = dims(window)
    xs = c[0] + (np.arange(nx, dtype=np.float64) - float((nx - 1) // 2)) * s[0]
    ys = c[1] + (np.arange(ny, dtype=np.float64) - float((ny - 1) // 2)) * s[1]
    if cyclic:
        th = c[2] + np.arange(nt, dtype=np.float64) * (2.0 * PI / float(nt))
    else:
        th = c[2] + (np.arange(nt, dtype=np.float64) - float((nt - 1) // 2)) * s[2]
    return xs, ys, wrap(th)


def _shift(a, d, axis, cyclic):
    """b[i] = a[i + d] along axis, and where that neighbour exists."""
    if cyclic:
        return np.roll(a, -d, axis=axis), np.ones(a.shape, dtype=bool)
    b = np.zeros_like(a)
    ok = np.zeros(a.shape, dtype=bool)
    n = a.shape[axis]
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if d > 0:
        src[axis], dst[axis] = slice(d, n), slice(0, max(n - d, 0))
    elif d < 0:
        src[axis], dst[axis] = slice(0, max(n + d, 0)), slice(-d, n)
    b[tuple(dst)] = a[tuple(src)]
    ok[tuple(dst)] = True
    return b, ok


def peaks(volume, cyclic: bool):
    """Mask of the lattice's peaks: score > 0 and beating every distinct in-window 3x3x3 neighbour (a higher score, or
    the same score and a lower flat index); theta neighbours wrap only on a cyclic axis."""
    v = np.asarray(volume, dtype=np.float32)
    idx = np.arange(v.size, dtype=np.int64).reshape(v.shape)
    peak = v > 0
    for dj in (-1, 0, 1):
        vj, okj = _shift(v, dj, 0, cyclic)
        ij, _ = _shift(idx, dj, 0, cyclic)
        for dy in (-1, 0, 1):
            vy, oky = _shift(vj, dy, 1, False)
            iy, _ = _shift(ij, dy, 1, False)
            oky &= _shift(okj, dy, 1, False)[0]
            for dx in (-1, 0, 1):
                if dj == dy == dx == 0:
                    continue
                vx, okx = _shift(vy, dx, 2, False)
                ix, _ = _shift(iy, dx, 2, False)
                okx &= _shift(oky, dx, 2, False)[0]
                beaten = okx & (ix != idx) & ((vx > v) | ((vx == v) & (ix < idx)))
                peak &= ~beaten
    return peak


def select_hits(volume, window, k: int = 8, min_sep=(0.5, 0.1)):
    """The hits of a score volume [n_theta, n_y, n_x]: the best min(#peaks, 4096) peaks by (score desc, index asc),
    walked in that order, each accepted unless an accepted hit lies closer than min_sep[0] in translation AND closer
    than min_sep[1] in wrapped heading; at most k.  A list of SearchHit."""
    (nt, ny, nx), cyclic = dims(window)
    v = np.asarray(volume, dtype=np.float32).reshape(nt, ny, nx)
    xs, ys, th = lattice(window)
    pinned = tuple(float(c) for c in window[0][2:5]) if len(window[0]) == 6 else None
    cand = np.flatnonzero(peaks(v, cyclic))
    sc = v.reshape(-1)[cand]
    order = np.lexsort((cand, -sc))[:SHORTLIST]
    st, sr = float(min_sep[0]), float(min_sep[1])
    st2 = st * st
    hits = []
    for q in cand[order]:
        if len(hits) >= k:
            break
        q = int(q)
        ix, iy, j = q % nx, (q // nx) % ny, q // (nx * ny)
        p = (float(xs[ix]), float(ys[iy]), float(th[j]))
        keep = True
        for hh in hits:
            dx, dy = p[0] - hh.pose[0], p[1] - hh.pose[1]
            dt = abs(float(wrap(p[2] - hh.pose[-1])))
            if dx * dx + dy * dy < st2 and dt < sr:
                keep = False
                break
        if keep:
            hits.append(SearchHit(p if pinned is None else (p[0], p[1], *pinned, p[2]), float(v.reshape(-1)[q]), q))
    return hits


def select_best(scores, poses, k: int = 8, min_sep=(0.5, 0.1)):
    """The hits of a scored pose list (docs/ALGORITHM.md "Scoring a list of poses"; ndt2d/ndt3d_best_poses_dev):
    scores [m] float32, poses [m, 3] = (x, y, theta) or [m, 6] = (tx, ty, tz, roll, pitch, yaw).  Candidates are the
    poses with score > 0; the best min(#candidates, 4096) by (score desc, index asc) are walked in that order, each
    accepted unless an accepted hit lies closer than min_sep[0] in translation (Euclidean over x, y, and z in 3D) AND
    closer than min_sep[1] in rotation (the wrapped heading difference; in 3D the largest of the wrapped roll, pitch and
    yaw differences), both strictly; at most k.  A list of SearchHit whose pose is the list's row, not wrapped."""
    v = np.asarray(scores, dtype=np.float32).reshape(-1)
    p = np.asarray(poses, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] not in (3, 6) or p.shape[0] != v.size:
        raise ValueError("poses is [m, 3] or [m, 6] with one row per score")
    nt = 2 if p.shape[1] == 3 else 3
    cand = np.flatnonzero(v > 0)
    order = np.lexsort((cand, -v[cand]))[:SHORTLIST]
    st, sr = float(min_sep[0]), float(min_sep[1])
    st2 = st * st
    hits = []
    for q in cand[order]:
        if len(hits) >= k:
            break
        q = int(q)
        row = tuple(float(c) for c in p[q])
        keep = True
        for hh in hits:
            d2 = 0.0
            for a in range(nt):
                d = row[a] - hh.pose[a]
                d2 = d2 + d * d
            dr = 0.0
            for a in range(nt, len(row)):
                dr = max(dr, abs(float(wrap(row[a] - hh.pose[a]))))
            if d2 < st2 and dr < sr:
                keep = False
                break
        if keep:
            hits.append(SearchHit(row, float(v[q]), q))
    return hits
