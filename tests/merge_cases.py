"""Scenes, poses and shared helpers of the submap-merge tests (test_map_merge_ref.py, test_gpu_merge_map.py,
test_gpu_merge_map3d.py).

Scenes are coarsen_cases.lattice_cloud clouds (coordinates on a 2^-11 lattice) in the SOURCE map's own frame.  "tiny" also has
one cell that holds a single point and one cell of five identical points off the lattice: a degenerate block, whose
n dSS_aa and dS_a^2 are equal before the roundings, so that the clamp of section 2.18 acts (the tests assert that it did).
The destination is a reserved extent around the source's with its own, different points."""
import math

import numpy as np

import coarsen_cases as K
import map_coarsen_ref as R

C2, C3 = 0.5, 1.0
SCENES2 = {"tiny": ((-7, -5), (13, 11), 300), "wide": ((-151, -101), (301, 201), 20000)}
SCENES3 = {"tiny": ((-3, -5, -2), (9, 8, 7), 3000), "wide": ((-21, -14, -5), (40, 30, 12), 60000)}
SINGLE2, CLUSTER2 = (0.3 + 2.0 ** -11, 0.2 + 2.0 ** -11), (1.8 + 2.0 ** -23, 1.8 + 5 * 2.0 ** -23)
SINGLE3, CLUSTER3 = (0.3 + 2.0 ** -11, 1.2 + 2.0 ** -11, 0.4 + 2.0 ** -11), (1.8 + 2.0 ** -23, 1.8 + 5 * 2.0 ** -23, 1.3 + 3 * 2.0 ** -23)
_cache = {}
TILTED = ("steep", "near_gimbal")              # the 3D poses with |roll|, |pitch| >= 0.5 rad


def points(dim, scene, seed=17):
    """The source cloud [n, dim] float32 of a scene."""
    key = (dim, scene, seed)
    if key not in _cache:
        k0, ext, n = (SCENES2 if dim == 2 else SCENES3)[scene]
        c = C2 if dim == 2 else C3
        tiny = scene == "tiny"
        pts = K.lattice_cloud(seed, k0, ext, c, n, (((0.0,) * dim, (2.0,) * dim) if tiny else None))
        if tiny:
            single, cluster = (SINGLE2, CLUSTER2) if dim == 2 else (SINGLE3, CLUSTER3)
            pts = np.vstack([pts, np.array(single)[None, :], np.repeat(np.array(cluster)[None, :], 5, axis=0)]).astype(np.float32)
        _cache[key] = pts
    return _cache[key]


def extent(dim, scene, margin):
    """(lo, hi) per axis of the scene's interior grown by `margin` metres: what the destination reserves."""
    k0, ext, _ = (SCENES2 if dim == 2 else SCENES3)[scene]
    c = C2 if dim == 2 else C3
    return [(k0[a] + 1) * c - margin for a in range(dim)], [(k0[a] + ext[a] - 1) * c + margin for a in range(dim)]


def own_points(dim, scene, n=200, seed=5):
    """Points of the destination's own, inside the scene's interior (no lattice: these go through the point kernels)."""
    lo, hi = extent(dim, scene, 0.0)
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, size=(n, dim)).astype(np.float32)


def poses(dim, scene):
    """name -> pose: identity, a whole-cell shift, a general pose, yaw within 1e-3 of +pi and of -pi, and one that puts part
    of the source outside the destination (in 2D part of it on the destination's ring).  3D also: "steep" and
    "near_gimbal", the attitudes of tilted_cases.ATTITUDES with translations like "general" - roll and pitch of 0.5 rad and
    more, where the sin roll sin pitch entries of R count (every other pose keeps them below 0.03)."""
    c = C2 if dim == 2 else C3
    if dim == 2:
        out = 4.3 if scene == "tiny" else 60.0
        return {"identity": (0.0, 0.0, 0.0), "shift": (2 * c, -3 * c, 0.0), "general": (0.3217, -0.1934, 0.7),
                "near_pi": (0.11, 0.07, math.pi - 7e-4), "near_minus_pi": (-0.13, 0.21, -math.pi + 4e-4),
                "partly_outside": (out, 0.37 * out, 0.05)}
    out = 4.3 if scene == "tiny" else 12.0
    return {"identity": (0.0,) * 6, "shift": (2 * c, -c, c, 0.0, 0.0, 0.0), "general": (0.3217, -0.1934, 0.2781, 0.11, -0.23, 0.7),
            "near_pi": (0.11, 0.07, -0.05, 0.0, 0.0, math.pi - 7e-4), "near_minus_pi": (-0.13, 0.21, 0.04, 0.02, -0.01, -math.pi + 4e-4),
            "partly_outside": (out, 0.37 * out, 0.4, 0.03, -0.02, 0.05),
            "steep": (0.2871, -0.2209, 0.3127, 0.7, -0.5, 2.1), "near_gimbal": (-0.3391, 0.1873, 0.2443, 1.2, 1.45, 0.4)}


def empty_blob(dim, c, origin, ext):
    """The blob of a reserved grid that holds no point."""
    return R.blob_from_points(np.zeros((0, dim), dtype=np.float32), c, origin, ext)[0]


def reserved_geometry(dim, lo, hi, c):
    """(origin float32 [dim], extents) ndt*_reserve_target derives from the box lo .. hi."""
    return R.grid_geometry(np.array([lo, hi], dtype=np.float32), c)


def fixed_units(pts, c, origin):
    """(cell index [n, dim], U int64 [n, dim]) of every point under blob_from_points' rule."""
    pts = np.asarray(pts, dtype=np.float32)
    origin = np.asarray(origin, dtype=np.float32)
    idx = ((pts - origin[None, :]) * np.float32(1.0 / c)).astype(np.int64)
    centre = R.cell_centres(origin, idx, c)
    return idx, np.rint((pts.astype(np.float64) - centre) * (2.0 ** 22 / c)).astype(np.int64)


# ---- the GPU tests' shared steps (2D and 3D differ in the matcher class and the number of coordinates) ---------------------
def matcher(dim, **params):
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D
    return (NdtMatcher2D if dim == 2 else NdtMatcher3D)(**params)


def cols(pts):
    return [np.ascontiguousarray(pts[:, a]) for a in range(pts.shape[1])]


def zero(dim):
    return (0.0,) * (3 if dim == 2 else 6)


def source(dim, scene, c=None, seed=17):
    """A matcher that holds the scene's cloud in its own frame (cell size c: the scene's, or half of the destination's)."""
    m = matcher(dim, cell_size=c or (C2 if dim == 2 else C3))
    m.set_target(*cols(points(dim, scene, seed)))
    return m


def destination(dim, scene, c=None, own=True, margin=2.0):
    """A matcher with a reserved extent around the scene (and points of its own), with an eig_ratio that is not the source's."""
    m = matcher(dim, cell_size=c or (C2 if dim == 2 else C3), eig_ratio=0.03)
    lo, hi = extent(dim, scene, margin)
    if dim == 2:
        m.reserve_target(lo[0], lo[1], hi[0], hi[1])
    else:
        m.reserve_target(lo, hi)
    if own:
        m.add_target_points(*cols(own_points(dim, scene)))
    return m


def moved(dim, pts, pose):
    """pts [n, dim] under `pose`, float64 arithmetic, float32 result (test input only: nothing compares with its bits)."""
    import map_merge_ref as M
    Rm, t = M.rotation(dim, pose)
    Rm = np.array(Rm)[:dim, :dim]
    return (pts.astype(np.float64) @ Rm.T + np.array(t[:dim])).astype(np.float32)


def scan_of(dim, scene, pose, n=400):
    """A small scan that fits the merged map: some of the source's points at `pose`, a few centimetres off."""
    pts = points(dim, scene)
    rng = np.random.default_rng(2)
    q = moved(dim, pts[rng.choice(len(pts), size=min(n, len(pts)), replace=False)], pose)
    return cols(q + np.float32(0.02))


def assert_is_a_loaded_handle(dim, dst, blob, scan, other_scene_pts):
    """dst is what a handle is after load_map(blob): same grid, same alignments on either side of a map-to-map call, and
    it takes points and gives them back."""
    with matcher(dim, cell_size=dst.params.cell_size, eig_ratio=0.03) as loaded, \
            matcher(dim, cell_size=dst.params.cell_size) as other:
        loaded.load_map(blob)
        K.same_grid(dst, loaded)
        K.same_result(dst.align(*scan, zero(dim)), loaded.align(*scan, zero(dim)))
        other.set_target(*cols(other_scene_pts))
        K.same_result(dst.align_map(other, zero(dim)), loaded.align_map(other, zero(dim)))
        K.same_result(other.align_map(dst, zero(dim)), other.align_map(loaded, zero(dim)))
    out_add = dst.add_target_points(*scan)
    assert not np.array_equal(dst.save_map(), blob)
    assert dst.remove_target_points(*scan) == out_add
    assert np.array_equal(dst.save_map(), blob)
