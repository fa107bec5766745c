"""The life of one matcher handle, as data: an exact model of what a handle holds as its target, and seeded schedules of
calls that walk a handle and its long-lived partner through every mutator and every query family
(tests/test_handle_life_ref.py checks the schedules on the model alone; tests/test_gpu_handle_life.py walks real handles).

THE MODEL (HandleModel): the target state of a handle with overlap_grids = 1, 2D or 3D, as the save_map blob defines it -
the lattice (float32 origin, extents), the per-cell integer sums, and in 2D n_points.  The sums ARE the multiset of binned
float32 points plus the integer contributions merged from other maps: every operation changes them by integer arithmetic
through the references the suite already owns (map_coarsen_ref.blob_from_points for points in a given lattice,
map_merge_ref.map_merge_ref, map_coarsen_ref.map_coarsen_ref), so after each operation model.blob() is the bytes save_map
must return, header included.  From the integers alone the model also predicts n_outside of every add, remove and merge,
n_valid (n >= max(min_points, 2) and a positive trace of n SS - S S': the integer rule of
cell_record_ref.exact_cells, which test_handle_life_ref.py compares it with), and which calls fail with which status:
  * a removal fails (NDT_ERR_INVALID_ARG) when a cell's count goes below zero, or reaches zero with a sum left;
  * a merge fails (NDT_ERR_CAPACITY) when a destination cell would pass 2^20 points;
  * after a failure the model has no target until the next set_target, reserve, load or coarsen_from.
n_points (2D) follows csrc: set_target counts every point it was given, an add / remove the points that were binned, a
merge the n it filed; load and coarsen carry the header's over; a reserve starts at 0.

THE SCHEDULES (schedule(dim, seed)): a list of steps, each a plain tuple (op, who, numpy arguments ...) with who = 0 for
the handle and 1 for its partner.  Mutators: set_target, reserve, add, remove, merge, unmerge, load, coarsen_from and, in
3D, set_neighbourhood.  Queries: QUERIES below; the map-to-map ones take the other handle as their source, so each handle
serves as target and as source.  Life.apply(step) replays a step on the two models."""
import math

import numpy as np

import map_coarsen_ref as R
import map_merge_ref as MM

NDT_OK, NDT_ERR_INVALID_ARG, NDT_ERR_NO_TARGET, NDT_ERR_CAPACITY = 0, -1, -2, -5        # include/ndt_hip.h
CELL = {2: 0.5, 3: 1.0}
MIN_POINTS = {2: 3, 3: 5}                      # ndt2d_default_params / ndt3d_default_params
NPOSE = {2: 3, 3: 6}
SCAN_SIZES = (1, 63, 64, 65, 1000, 4096, 4097, 8191)       # both sides of a wave and of the 4096-point short-scan limit
TARGET_SIZES = (300, 3000, 20000)
MUTATORS = ("set_target", "reserve", "add", "remove", "merge", "unmerge", "load", "coarsen_from")
POINT_QUERIES = ("align", "align_host", "align_async", "align_trace", "evaluate", "multi_start", "multi_scan", "score_poses",
                 "score_particles", "search_align", "fit_points", "select_points")
MAP_QUERIES = ("align_map", "align_map_multi", "score_map_poses", "search_align_map")
QUERIES = POINT_QUERIES + MAP_QUERIES
SINGLE_VOXEL_ONLY = ("score_poses", "score_particles", "search_align", "fit_points", "select_points")    # refused with neighbourhood 7


# ---- a scan moved into the map frame, as the device does it -------------------------------------------------------------
def moved2d(x, y, pose):
    """ndt2d_add_target_points_dev's float32 restatement (tests/test_gpu_scan_sequence.py pins it to the device's)."""
    c, s = np.float32(math.cos(pose[2])), np.float32(math.sin(pose[2]))
    return ((c * x - s * y) + np.float32(pose[0])).astype(np.float32), ((s * x + c * y) + np.float32(pose[1])).astype(np.float32)


def moved3d(x, y, z, pose):
    """ndt3d_add_target_points_dev's float32 restatement (tests/test_gpu_scan_sequence3d.py pins it to the device's)."""
    from gtsam_ndt_amd import synth3d
    R3 = synth3d.rotation(*pose[3:]).astype(np.float32)
    t = np.asarray(pose[:3], np.float32)
    out = []
    for r in range(3):
        a, b, c = R3[r, 0] * x, R3[r, 1] * y, R3[r, 2] * z
        out.append((((a + b) + c) + t[r]).astype(np.float32))
    return out


def moved(pts, pose):
    """pts [n, dim] float32 -> [n, dim] float32 at `pose` (None: as they are)."""
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    if pose is None:
        return pts
    cols = [np.ascontiguousarray(pts[:, a]) for a in range(pts.shape[1])]
    with np.errstate(invalid="ignore", over="ignore"):
        out = moved2d(*cols, pose) if pts.shape[1] == 2 else moved3d(*cols, pose)
    return np.stack(out, axis=1)


# ---- the model ----------------------------------------------------------------------------------------------------------
class HandleModel:
    def __init__(self, dim, cell_size=None, min_points=None):
        self.dim = dim
        self.c = float(cell_size if cell_size is not None else CELL[dim])
        self.min_points = int(min_points if min_points is not None else MIN_POINTS[dim])
        self.has_target = False
        self.h = self.cells = None

    # -- state
    def _install(self, blob):
        h, cells = R.parse(blob)
        assert h["dims"] == self.dim and h["ngrid"] == 1 and h["cell_size"] == self.c
        self.h, self.cells, self.has_target = h, cells.copy(), True

    def _fail(self, status):
        self.has_target, self.h, self.cells = False, None, None
        return status, None

    @property
    def origin(self):
        return np.asarray(self.h["origin"], dtype=np.float32)[0, :self.dim]

    @property
    def ext(self):
        return [self.h["width"], self.h["height"], self.h["depth"]][:self.dim]

    def blob(self):
        """The bytes save_map must return."""
        assert self.has_target
        return R.pack(self.h, self.cells)

    def n_points(self):
        return int(self.h["n_points"])

    def n_valid(self):
        n = self.cells["n"].astype(np.int64)
        k = np.flatnonzero(n >= max(self.min_points, 2))
        nn = n[k].astype(object)
        trace = 0
        for a in range(self.dim):
            p = MM.pairs_of(self.dim).index((a, a))
            s = self.cells["s"][k, a].astype(object)
            trace = trace + (nn * self.cells["ss"][k, p].astype(object) - s * s)
        return int(np.count_nonzero(trace > 0)) if k.size else 0

    def max_count(self):
        return int(self.cells["n"].max()) if self.has_target and self.cells.size else 0

    # -- lattice (csrc/ndt_lattice.hpp cell_of: RING = 1 in 2D, 0 in 3D; a NaN or an infinity is outside)
    def inside(self, pts):
        ring = np.float32(1 if self.dim == 2 else 0)
        with np.errstate(invalid="ignore", over="ignore"):
            f = (np.asarray(pts, dtype=np.float32) - self.origin[None, :]) * np.float32(1.0 / self.c)
            ok = np.ones(len(pts), dtype=bool)
            for a in range(self.dim):
                ok &= (f[:, a] >= ring) & (f[:, a] < np.float32(self.ext[a]) - ring)
        return ok

    def _sums_of(self, pts):
        """The structured cells of the points (all inside) binned into this lattice."""
        return R.parse(R.blob_from_points(pts, self.c, self.origin, self.ext)[0])[1]

    # -- mutators: each returns (status, n_outside)
    def set_target(self, pts):
        pts = np.asarray(pts, dtype=np.float32)
        fin = pts[np.isfinite(pts).all(axis=1)]
        self._install(R.blob_from_points(fin, self.c)[0])
        self.h["n_points"] = len(pts) if self.dim == 2 else 0
        return NDT_OK, None

    def reserve(self, lo, hi):
        origin, ext = R.grid_geometry(np.array([lo, hi], dtype=np.float32), self.c)
        self._install(R.blob_from_points(np.zeros((0, self.dim), np.float32), self.c, origin, ext)[0])
        return NDT_OK, None

    def _update(self, pts, pose, sign):
        if not self.has_target:
            return NDT_ERR_NO_TARGET, None
        w = moved(pts, pose)
        ok = self.inside(w)
        d = self._sums_of(w[ok])
        n = self.cells["n"].astype(np.int64) + sign * d["n"].astype(np.int64)
        s = self.cells["s"] + sign * d["s"]
        ss = self.cells["ss"] + sign * d["ss"]
        if sign < 0 and (np.any(n < 0) or np.any((n == 0) & (np.any(s != 0, axis=1) | np.any(ss != 0, axis=1)))):
            return self._fail(NDT_ERR_INVALID_ARG)
        if n.max(initial=0) > R.MAX_CELL_COUNT:
            return self._fail(NDT_ERR_CAPACITY)
        self.cells["n"], self.cells["s"], self.cells["ss"] = n.astype(np.uint32), s, ss
        if self.dim == 2:
            self.h["n_points"] += sign * int(ok.sum())
        return NDT_OK, int(len(w) - ok.sum())

    def add(self, pts, pose=None):
        return self._update(pts, pose, 1)

    def remove(self, pts, pose=None):
        return self._update(pts, pose, -1)

    def _merge(self, src_blob, pose, sign):
        if not self.has_target:
            return NDT_ERR_NO_TARGET, None
        out, n_outside = MM.map_merge_ref(self.blob(), src_blob, pose, sign)
        h, cells = R.parse(out)
        n = cells["n"]
        if sign < 0 and (np.any(n > R.MAX_CELL_COUNT) or                      # (a count below zero wraps, as on the device)
                         np.any((n == 0) & (np.any(cells["s"] != 0, axis=1) | np.any(cells["ss"] != 0, axis=1)))):
            return self._fail(NDT_ERR_INVALID_ARG)
        if np.any(n > R.MAX_CELL_COUNT):
            return self._fail(NDT_ERR_CAPACITY)
        self.h, self.cells = h, cells.copy()
        return NDT_OK, n_outside

    def merge(self, src_blob, pose):
        return self._merge(src_blob, pose, 1)

    def unmerge(self, src_blob, pose):
        return self._merge(src_blob, pose, -1)

    def load(self, blob):
        self._install(blob)
        return NDT_OK, None

    def coarsen_from(self, fine_blob):
        self._install(R.map_coarsen_ref(fine_blob, int(round(self.c / R.parse(fine_blob)[0]["cell_size"]))))
        return NDT_OK, None


def fine_blob(dim, fine_pts, f):
    """What a handle of cell size CELL / f saves after set_target(fine_pts): the source of a coarsen_from step."""
    m = HandleModel(dim, CELL[dim] / f)
    m.set_target(fine_pts)
    return m.blob()


def forged_source(dim):
    """The 2^19-point-cell blob of tests/test_gpu_merge_map.py, at this file's cell size."""
    from test_gpu_merge_map import _forged_source
    return _forged_source(dim, CELL[dim])


class Life:
    """The two models of a schedule.  apply(step) -> dict(kind, status, n_outside): what the call must answer."""

    def __init__(self, dim):
        self.dim = dim
        self.model = [HandleModel(dim), HandleModel(dim)]
        self.neighbourhood = [1, 1]

    def involved(self, step):
        op, who = step[0], step[1]
        return (who, 1 - who) if op in MAP_QUERIES else (who,)

    def apply(self, step):
        op, who = step[0], step[1]
        m = self.model[who]
        if op in QUERIES:
            ok = all(self.model[w].has_target for w in self.involved(step))
            return dict(kind="query", status=NDT_OK if ok else NDT_ERR_NO_TARGET, n_outside=None)
        if op == "set_neighbourhood":
            self.neighbourhood[who] = int(step[2])
            return dict(kind="setting", status=NDT_OK, n_outside=None)
        if op == "coarsen_from":
            st, out = m.coarsen_from(fine_blob(self.dim, step[2], int(step[3])))
        else:
            st, out = getattr(m, op)(*step[2:])
        return dict(kind="mutator", status=st, n_outside=out)


# ---- clouds, scans, poses -----------------------------------------------------------------------------------------------
def _cloud(rng, dim, n, centre, size, with_inf):
    """n points [n, dim] float32 of a room `size` metres across round `centre`: walls (and a floor in 3D) with 2 cm noise,
    no-return points (NaN) and, with_inf, one infinity."""
    u = rng.uniform(-0.5, 0.5, n) * size
    side = rng.integers(0, 4 if dim == 2 else 6, n)
    half = 0.5 * size
    x = np.where(side == 0, -half, np.where(side == 1, half, u))
    y = np.where(side == 2, -half * 0.8, np.where(side == 3, half * 0.8, np.where(side < 2, u * 0.8, rng.uniform(-0.4, 0.4, n) * size)))
    cols = [x, y]
    if dim == 3:
        cols.append(np.where(side >= 4, 0.0, rng.uniform(0.0, 3.0, n)))
    p = np.stack(cols, axis=1) + rng.normal(0.0, 0.02, (n, dim)) + np.asarray(centre)[None, :]
    p = p.astype(np.float32)
    if n > 50:
        p[::97, 0] = np.nan
        if with_inf:
            p[n // 2, 1] = np.inf
    return p


def _small_pose(rng, dim, trans, rot):
    if dim == 2:
        return np.concatenate([rng.uniform(-trans, trans, 2), rng.uniform(-rot, rot, 1)])
    return np.concatenate([rng.uniform(-trans, trans, 3), rng.uniform(-rot, rot, 3) * [0.2, 0.2, 1.0]])


def _sensor_frame(dim, world, pose):
    """The finite world points [n, dim] seen from `pose` (float64; test input only: nothing compares with its bits)."""
    Rm, t = MM.rotation(dim, pose)
    Rm = np.array(Rm)[:dim, :dim]
    return (world.astype(np.float64) - np.array(t[:dim])[None, :]) @ Rm          # R' (w - t)


class _Gen:
    def __init__(self, dim, seed):
        self.dim, self.rng = dim, np.random.default_rng([dim, seed])
        self.life = Life(dim)
        self.steps = []
        self.scene = [None, None]              # finite world points the handle's map is made of (for scans that hit)
        self.good = [None, None]               # the blob after the last mutator that went well

    def emit(self, *step):
        step = tuple(step)
        out = self.life.apply(step)
        self.steps.append(step)
        who = step[1]
        if out["kind"] == "mutator" and out["status"] == NDT_OK:
            self.good[who] = self.life.model[who].blob()
        return out

    # -- inputs
    def cloud(self, n, far=False, size=None):
        rng = self.rng
        centre = rng.uniform(-300, 300, self.dim) if far else rng.uniform(-3, 3, self.dim)
        if self.dim == 3:
            centre[2] = rng.uniform(-2, 2)
        size = size or float(rng.choice([12.0, 24.0, 40.0]))
        return _cloud(rng, self.dim, n, centre, size, with_inf=self.dim == 2)

    def scan(self, who, n, noise=0.01):
        """(scan [n, dim] float32 in a sensor frame, the pose that puts it on the map, a start pose near it)."""
        rng, dim = self.rng, self.dim
        world = self.scene[who]
        centre = world.mean(axis=0)
        true = _small_pose(rng, dim, 0.5, 0.05)
        true[:dim] += centre
        pick = world[rng.integers(0, len(world), n)]
        s = (_sensor_frame(dim, pick, true) + rng.normal(0.0, noise, (n, dim))).astype(np.float32)
        if n >= 63:
            s[5, 0] = np.nan
            s[n // 3, dim - 1] = np.inf
        return s, true, true + _small_pose(rng, dim, 0.08, 0.01)

    def scan_size(self):
        return int(self.rng.choice(SCAN_SIZES))

    def starts(self, pose, m):
        return np.stack([pose + _small_pose(self.rng, self.dim, 0.15, 0.02) for _ in range(m)])

    def multi_m(self):
        rng = self.rng
        return int(rng.choice([1, 2, 6, 7, 11, 12, 13, 16, 17, 32, 33, 64])) if rng.random() < 0.6 else int(rng.integers(1, 65))

    def map_pose(self, who):
        """A start for aligning the other handle's map to this one's: the other's scene moved onto this one's, nearly."""
        pose = _small_pose(self.rng, self.dim, 0.1, 0.01)
        pose[:self.dim] += self.scene[who].mean(axis=0) - self.scene[1 - who].mean(axis=0)
        return pose

    def set_scene(self, who, pts):
        self.scene[who] = pts[np.isfinite(pts).all(axis=1)]

    # -- queries
    def query(self, op, who):
        rng, dim = self.rng, self.dim
        if op in ("align", "align_host"):
            n = {"align": int(rng.choice([4097, 8191, 1000])), "align_host": int(rng.choice([1, 63, 64, 65, 4096]))}[op]
            s, _, init = self.scan(who, n)
            self.emit(op, who, s, init)
        elif op == "align_async":
            run = int(rng.integers(1, 5))
            big = [int(rng.choice([4097, 8191])) for _ in range(run)]
            if rng.random() < 0.3:
                big[-1] = int(rng.choice([65, 1000, 4096]))         # a short scan at the end of a run of long ones
            scans = [self.scan(who, n) for n in big]
            self.emit(op, who, [s[0] for s in scans], np.stack([s[2] for s in scans]))
        elif op == "align_trace":
            s, _, init = self.scan(who, int(rng.choice([65, 1000, 4097])))
            self.emit(op, who, s, init)
        elif op == "evaluate":
            s, true, _ = self.scan(who, self.scan_size())
            self.emit(op, who, s, true)
        elif op == "multi_start":
            s, _, init = self.scan(who, int(rng.choice([1000, 4096, 4097, 8191])))
            self.emit(op, who, s, self.starts(init, self.multi_m()))
        elif op == "multi_scan":
            m = self.multi_m()
            scans = [self.scan(who, self.scan_size() if k < 8 else int(rng.choice([63, 65, 1000]))) for k in range(m)]
            self.emit(op, who, [s[0] for s in scans], np.stack([s[2] for s in scans]))
        elif op in ("score_poses", "score_particles"):
            s, true, _ = self.scan(who, self.scan_size())
            poses = self.starts(true, int(rng.choice([1, 63, 64, 65, 300])))
            poses[-1, 0] = np.nan                                  # a pose that is not finite scores 0
            self.emit(op, who, s, poses)
        elif op == "search_align":
            s, true, _ = self.scan(who, int(rng.choice([1000, 4097])))
            self.emit(op, who, s, true, np.array([1.0, 1.0, 0.1]), np.array([0.5, 0.5, 0.05]), 4)
        elif op in ("fit_points", "select_points"):
            s, true, _ = self.scan(who, self.scan_size(), noise=0.05)
            self.emit(op, who, s, true, 9.0)
        elif op == "align_map":
            self.emit(op, who, self.map_pose(who))
        elif op == "align_map_multi":
            self.emit(op, who, self.starts(self.map_pose(who), int(rng.choice([1, 2, 5, 9, 17, 33]))))
        elif op == "score_map_poses":
            self.emit(op, who, self.starts(self.map_pose(who), int(rng.choice([1, 65, 200]))))
        elif op == "search_align_map":
            centre = np.zeros(NPOSE[dim])
            centre[:dim] = self.scene[who].mean(axis=0) - self.scene[1 - who].mean(axis=0)
            self.emit(op, who, centre, np.array([1.0, 1.0, 0.1]), np.array([0.5, 0.5, 0.05]), 3)
        else:
            raise KeyError(op)

    def queries(self, count, who=None, only=None):
        """`count` queries, on `who` or on whichever handle the pool names.  The pool holds every family once per handle,
        in seeded order; a query that the moment does not admit (neighbourhood 7) waits in it; once it is empty the draws
        are random."""
        for _ in range(count):
            def admissible(op, w):
                return ((only is None or op in only) and (who is None or w == who)
                        and not (self.life.neighbourhood[w] == 7 and op in SINGLE_VOXEL_ONLY))
            ok = [k for k, (op, w) in enumerate(self.pool) if admissible(op, w)]
            if ok:
                op, w = self.pool.pop(ok[0])
            else:
                w = who if who is not None else int(self.rng.integers(0, 2))
                op = str(self.rng.choice([op for op in (only or QUERIES) if admissible(op, w)]))
            self.query(op, w)

    def fresh_pool(self):
        pool = [(op, who) for op in QUERIES for who in (0, 1)]
        return [pool[int(j)] for j in self.rng.permutation(len(pool))]

    # -- an empty cell well inside a handle's grid, as per-axis indices
    def empty_cell(self, who):
        m = self.life.model[who]
        ext = m.ext
        n = m.cells["n"].reshape(ext[::-1])
        inner = n[tuple(slice(2, e - 2) for e in ext[::-1])]
        free = np.argwhere(inner == 0)
        assert len(free), "no empty cell inside the grid"
        idx = free[int(self.rng.integers(0, len(free)))] + 2
        return [int(v) for v in idx[::-1]]                         # x, y (, z)

    def points_in_cell(self, who, idx, n):
        m = self.life.model[who]
        lo = m.origin.astype(np.float64) + np.array(idx) * m.c
        return (lo[None, :] + self.rng.uniform(0.2, 0.8, (n, self.dim)) * m.c).astype(np.float32)

    # -- blocks: a mutation of `who` and the queries behind it
    def b_rebuild(self, who, n, far):
        c = self.cloud(n, far)
        self.emit("set_target", who, c)
        self.set_scene(who, c)
        self.queries(1, who)

    def b_reserve_add(self, who):
        c = self.cloud(int(self.rng.choice([3000, 8000])), size=24.0)
        fin = c[np.isfinite(c).all(axis=1)]
        self.emit("reserve", who, fin.min(axis=0) - 3.0, fin.max(axis=0) + 3.0)
        self.emit("add", who, c[: len(c) // 2], None)                         # host arrays, already in the map frame
        rest = c[len(c) // 2:]
        pose = _small_pose(self.rng, self.dim, 1.0, 0.3)
        seen = _sensor_frame(self.dim, np.nan_to_num(rest, nan=0.0, posinf=0.0), pose).astype(np.float32)
        seen[~np.isfinite(rest).all(axis=1)] = np.nan
        self.emit("add", who, seen, pose)                                     # on the device, moved by a pose
        self.set_scene(who, c)
        self.queries(2, who)

    def b_add_remove(self, who, reanchor):
        n = int(self.rng.choice([65, 1000, 4097]))
        s, true, _ = self.scan(who, n)
        self.emit("add", who, s, true)
        self.queries(1)
        self.emit("remove", who, s, true)
        if reanchor:
            self.emit("add", who, s, true + _small_pose(self.rng, self.dim, 0.2, 0.02))
        self.queries(1, who)

    def b_merge_unmerge(self, who):
        src = self.cloud(int(self.rng.choice([300, 3000])), size=12.0)
        src -= np.nanmean(np.where(np.isfinite(src), src, np.nan), axis=0).astype(np.float32)[None, :]
        other = HandleModel(self.dim)
        other.set_target(src)
        pose = _small_pose(self.rng, self.dim, 0.5, 0.2)
        pose[:self.dim] += self.scene[who].mean(axis=0)
        src_blob = other.blob()
        self.emit("merge", who, src_blob, pose)
        self.queries(1)
        out = self.emit("unmerge", who, src_blob, pose)
        assert out["status"] == NDT_OK
        self.queries(1, who)

    def b_load(self, who, own):
        if own:
            self.emit("load", who, self.good[who])                            # what it saved itself
        else:
            c = self.cloud(int(self.rng.choice(TARGET_SIZES[:2])), far=bool(self.rng.integers(0, 2)))
            m = HandleModel(self.dim)
            m.set_target(c)
            self.emit("load", who, m.blob())
            self.set_scene(who, c)
        self.queries(1, who)

    def b_coarsen(self, who, f):
        c = self.cloud(int(self.rng.choice([3000, 8000])), size=float(self.rng.choice([12.0, 24.0])))
        self.emit("coarsen_from", who, c, f)
        self.set_scene(who, c)
        self.queries(1, who)

    def after_failure(self, who):
        """Queries that must answer NDT_ERR_NO_TARGET (drawn, not taken off the pool: they exercise no family), the last
        good map loaded again, and work on it."""
        ops = [op for op in POINT_QUERIES if not (self.life.neighbourhood[who] == 7 and op in SINGLE_VOXEL_ONLY)]
        self.query(str(self.rng.choice(ops)), who)
        self.query(str(self.rng.choice(MAP_QUERIES)), 1 - who)                # the partner, with this one as its source
        self.emit("load", who, self.good[who])
        self.queries(1, who)

    def b_bad_remove(self, who, kind):
        idx = self.empty_cell(who)
        p = self.points_in_cell(who, idx, 50)
        if kind == 0:                                                         # never added: a count goes below zero
            out = self.emit("remove", who, p, None)
        else:                                                                 # added, then removed 1 mm off: zero count, sums left
            self.emit("add", who, p, None)
            q = p.copy()
            q[:, 0] += np.float32(0.001)
            out = self.emit("remove", who, q, None)
        assert out["status"] == NDT_ERR_INVALID_ARG
        self.after_failure(who)

    def b_capacity(self, who):
        m = self.life.model[who]
        idx = self.empty_cell(who)
        pose = np.zeros(NPOSE[self.dim])
        pose[:self.dim] = m.origin.astype(np.float64) + (np.array(idx) + 0.5) * m.c
        forged = forged_source(self.dim)
        for _ in range(3):
            out = self.emit("merge", who, forged, pose)
        assert out["status"] == NDT_ERR_CAPACITY
        self.after_failure(who)

    def b_neighbourhood(self, who):
        self.emit("set_neighbourhood", who, 7)
        self.queries(3, who, only=("align", "evaluate", "align_trace", "multi_start", "multi_scan", "align_async"))
        self.emit("set_neighbourhood", who, 1)
        self.queries(1, who)

    def run(self):
        rng = self.rng
        self.pool = self.fresh_pool()
        # both handles get a target first; everything else comes in seeded order
        for who, n in ((0, 20000), (1, 3000)):
            c = self.cloud(n)
            self.emit("set_target", who, c)
            self.set_scene(who, c)
        self.queries(2, 0)
        self.queries(2, 1)
        blocks = [lambda: self.b_rebuild(0, 300, True), lambda: self.b_rebuild(0, 20000, False),
                  lambda: self.b_rebuild(1, 20000, True),
                  lambda: self.b_reserve_add(0), lambda: self.b_reserve_add(1),
                  lambda: self.b_add_remove(0, True), lambda: self.b_add_remove(1, False),
                  lambda: self.b_merge_unmerge(0), lambda: self.b_merge_unmerge(1),
                  lambda: self.b_load(0, True), lambda: self.b_load(1, False),
                  lambda: self.b_coarsen(0, 2), lambda: self.b_coarsen(1, 4),
                  lambda: self.b_bad_remove(0, 0), lambda: self.b_bad_remove(1, 1),
                  lambda: self.b_capacity(0), lambda: self.b_capacity(1)]
        if self.dim == 3:
            blocks += [lambda: self.b_neighbourhood(0), lambda: self.b_neighbourhood(1)]
        for j in rng.permutation(len(blocks)):
            blocks[int(j)]()
        while self.pool:                                                      # the families the blocks did not get to
            self.queries(1)
        return self.steps


_schedules = {}


def schedule(dim, seed):
    """The steps of one life (cached: the tests share them and leave them unchanged)."""
    if (dim, seed) not in _schedules:
        _schedules[(dim, seed)] = _Gen(dim, seed).run()
    return _schedules[(dim, seed)]


def short_schedule(seed):
    """A 2D life without map-to-map calls, merges, loads of foreign maps or coarsening, for the overlap_grids = 4 run: the
    truth for its state is a rebuild from points (reserve + adds), which this schedule keeps possible."""
    g = _Gen(2, 1000 + seed)
    g.pool = [(str(op), 0) for op in g.rng.permutation(POINT_QUERIES)]
    c = g.cloud(8000, size=24.0)
    fin = c[np.isfinite(c).all(axis=1)]
    g.emit("reserve", 0, fin.min(axis=0) - 3.0, fin.max(axis=0) + 3.0)
    g.emit("add", 0, c, None)
    g.set_scene(0, c)
    g.queries(3, 0)
    g.b_add_remove(0, True)
    g.queries(2, 0)
    g.b_add_remove(0, False)
    g.queries(3, 0)
    return g.steps
