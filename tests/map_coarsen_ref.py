"""Reference for ndt2d_coarsen_map / ndt3d_coarsen_map (docs/ALGORITHM.md section 2.17) in Python integers: a save_map blob
and a factor -> the blob the coarser handle saves.  Everything is integer arithmetic, so there is exactly one right
answer; the GPU tests compare byte for byte, header included.

Blob layout (include/ndt_hip.h, ndt_map_header): 104 header bytes, then per cell DIM int64 first sums, DIM (DIM + 1) / 2
int64 second sums (xx xy yy | xx xy xz yy yz zz), uint32 n, uint32 pad - x fastest, then y, then z."""
import struct
from fractions import Fraction

import numpy as np

MAGIC = 0x4D54444E
HEADER = struct.Struct("<IIiiiiiIdQQ12f")          # 104 bytes
MAX_CELL_COUNT = 1 << 20
MAX_CELLS = 1 << 27
assert HEADER.size == 104


class CoarsenError(ValueError):
    pass


def cell_dtype(dim):
    npair = dim * (dim + 1) // 2
    return np.dtype([("s", "<i8", (dim,)), ("ss", "<i8", (npair,)), ("n", "<u4"), ("pad", "<u4")])


def parse(blob):
    """blob -> (header dict, structured cell array [n_cells])."""
    blob = np.ascontiguousarray(blob).view(np.uint8)
    if blob.size < HEADER.size:
        raise CoarsenError("shorter than a header")
    v = HEADER.unpack(blob[:HEADER.size].tobytes())
    h = dict(magic=v[0], version=v[1], dims=v[2], ngrid=v[3], width=v[4], height=v[5], depth=v[6], cell_bytes=v[7],
             cell_size=v[8], n_cells=v[9], n_points=v[10], origin=np.array(v[11:], dtype=np.float32).reshape(4, 3))
    if h["magic"] != MAGIC or h["version"] != 1 or h["dims"] not in (2, 3):
        raise CoarsenError("not an NDT map")
    dt = cell_dtype(h["dims"])
    if h["cell_bytes"] != dt.itemsize or h["n_cells"] != h["width"] * h["height"] * h["depth"] * h["ngrid"]:
        raise CoarsenError("header and cell blocks disagree")
    if blob.size < HEADER.size + h["n_cells"] * dt.itemsize:
        raise CoarsenError("blob is cut short")
    cells = np.frombuffer(blob[HEADER.size:HEADER.size + h["n_cells"] * dt.itemsize].tobytes(), dtype=dt)
    return h, cells


def pack(h, cells):
    o = np.asarray(h["origin"], dtype=np.float32).reshape(12)
    head = HEADER.pack(h["magic"], h["version"], h["dims"], h["ngrid"], h["width"], h["height"], h["depth"], h["cell_bytes"],
                       h["cell_size"], h["n_cells"], h["n_points"], *[float(x) for x in o])
    return np.frombuffer(head + cells.tobytes(), dtype=np.uint8).copy()


def coarsen_axis(origin, c, w, f):
    """(k0, K0, off, extent) of one axis: fine cell ix lies in coarse cell (off + ix) // f at position (off + ix) % f."""
    k0 = int(np.rint(float(origin) / c))
    K0 = f * ((k0 + 1 - f) // f)                       # floor division
    off = k0 - K0
    return k0, K0, off, (off + w - 2) // f + 2


def coarsen_cells(cells, dims, ext, offs, f, clamp=True):
    """The sums of section 2.17: structured fine cells [prod(ext)] -> (coarse extents, structured coarse cells)."""
    dim = dims
    pairs = [(a, b) for a in range(dim) for b in range(a, dim)]
    lg = {2: 1, 4: 2}[f]
    cext = [(offs[a] + ext[a] - 2) // f + 2 for a in range(dim)]
    acc = {}
    for k in np.flatnonzero(cells["n"]):
        k = int(k)
        idx = [k % ext[0], (k // ext[0]) % ext[1]] + ([k // (ext[0] * ext[1])] if dim == 3 else [])
        par = tuple((offs[a] + idx[a]) // f for a in range(dim))
        d = [(2 * ((offs[a] + idx[a]) % f) - f + 1) << 21 for a in range(dim)]
        n = int(cells["n"][k])
        s = [int(x) for x in cells["s"][k]]
        ss = [int(x) for x in cells["ss"][k]]
        e = acc.setdefault(par, [0, [0] * dim, [0] * len(pairs)])
        e[0] += n
        for a in range(dim):
            e[1][a] += s[a] + n * d[a]
        for p, (a, b) in enumerate(pairs):
            e[2][p] += ss[p] + d[a] * s[b] + d[b] * s[a] + n * d[a] * d[b]
    ncell = int(np.prod(cext))
    if ncell > MAX_CELLS:
        raise CoarsenError("more than 2^27 coarse cells")
    out = np.zeros(ncell, dtype=cell_dtype(dim))
    for par, (n, n1, n2) in acc.items():
        if n > MAX_CELL_COUNT:
            raise CoarsenError("a coarse cell holds more than 2^20 points")
        s = [(v + f // 2) >> lg for v in n1]
        ss = [(v + f * f // 2) >> (2 * lg) for v in n2]
        for p, (a, b) in enumerate(pairs):
            if clamp and a == b and n * ss[p] - s[a] * s[a] < 0:
                ss[p] = -((-s[a] * s[a]) // n)          # ceil(s^2 / n)
        k = par[0] + cext[0] * (par[1] + (cext[1] * par[2] if dim == 3 else 0))
        out["n"][k] = n
        out["s"][k] = s
        out["ss"][k] = ss
    return cext, out


def map_coarsen_ref(blob, f, clamp=True):
    """save_map(src) -> save_map(dst) for dst.cell_size = f * src.cell_size, f in (2, 4).  clamp=False leaves the
    degenerate-cell clamp out (for the test that shows it is needed)."""
    if f not in (2, 4):
        raise CoarsenError("the factor is 2 or 4")
    h, cells = parse(blob)
    if h["ngrid"] != 1:
        raise CoarsenError("overlapping grids do not coarsen")
    dim, c = h["dims"], h["cell_size"]
    ext = [h["width"], h["height"], h["depth"]][:dim]
    ax = [coarsen_axis(h["origin"][0][a], c, ext[a], f) for a in range(dim)]
    cext, out = coarsen_cells(cells, dim, ext, [a[2] for a in ax], f, clamp)
    g = dict(h)
    g["cell_size"] = f * c
    g["width"], g["height"] = cext[0], cext[1]
    g["depth"] = cext[2] if dim == 3 else 1
    g["n_cells"] = out.size
    origin = np.zeros((4, 3), dtype=np.float32)
    if dim == 2:                                       # the four origins ndt2d_set_target writes, also with one grid
        for q, (sx, sy) in enumerate(((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5))):
            origin[q, 0] = np.float32((ax[0][1] - sx * f) * c)
            origin[q, 1] = np.float32((ax[1][1] - sy * f) * c)
    else:
        origin[0] = [np.float32(a[1] * c) for a in ax]
    g["origin"] = origin
    return pack(g, out)


def cell_sums_plausible(n, s, ss_diag, ss_off):
    """ndt_map_io.hpp cell_sums_plausible: what ndt*_load_map accepts as the sums of a cell."""
    if n > MAX_CELL_COUNT:
        return False
    lim1, lim2 = n << 22, n << 44
    for su, suu in zip(s, ss_diag):
        if abs(su) > lim1 or suu < 0 or suu > lim2 or n * suu - su * su < 0:
            return False
    return all(abs(v) <= lim2 for v in ss_off)


# ---- fine blobs from points, in numpy, by the documented formula ------------------------------------------------------
def grid_geometry(pts, c):
    """ndt*_set_target's lattice for the cloud pts [n, dim] (float32 values): origin (float32) and extents per axis."""
    pts = np.asarray(pts, dtype=np.float32)
    origin, ext = [], []
    for a in range(pts.shape[1]):
        o = np.float32((np.floor(float(pts[:, a].min()) / c) - 1.0) * c)
        fx = np.float32(np.float32(pts[:, a].max() - o) * np.float32(1.0 / c))
        origin.append(o)
        ext.append(int(np.floor(float(fx))) + 2)
    return np.array(origin, dtype=np.float32), ext


def cell_centres(origin, idx, c):
    """float64 centres fma(i + 0.5, c, o) [n, dim] of the cells idx [n, dim] (cell_centre, csrc/ndt_lattice.hpp): the sum is
    formed exactly, as a fraction, and rounded once.  o + (i + 0.5) c in float64 rounds twice and moves the residual of a
    point in a hundred by one unit."""
    idx = np.asarray(idx, dtype=np.int64)
    fc = Fraction(float(c))
    out = np.zeros(idx.shape)
    for a in range(idx.shape[1]):
        fo = Fraction(float(np.float32(origin[a])))
        once = {int(i): float(Fraction(2 * int(i) + 1, 2) * fc + fo) for i in np.unique(idx[:, a])}
        out[:, a] = [once[int(i)] for i in idx[:, a]]
    return out


def blob_from_points(pts, c, origin=None, ext=None):
    """The blob ndt*_set_target + ndt*_save_map give for the cloud (float32 binning as the kernels:
    f = (p - o) * (float)(1 / c), cell = (int)f; U = rint((p - centre) 2^22 / c) with centre = fma(i + 0.5, c, o) in double).
    origin / ext: bin into this lattice instead of the cloud's own (ndt*_reserve_target + add_target_points)."""
    pts = np.asarray(pts, dtype=np.float32)
    dim = pts.shape[1]
    if origin is None:
        origin, ext = grid_geometry(pts, c)
    origin = np.asarray(origin, dtype=np.float32)
    inv_c = np.float32(1.0 / c)
    fidx = (pts - origin[None, :]) * inv_c                                  # float32
    idx = fidx.astype(np.int64)
    centre = cell_centres(origin, idx, c)
    U = np.rint((pts.astype(np.float64) - centre) * (2.0 ** 22 / c)).astype(np.int64)
    pairs = [(a, b) for a in range(dim) for b in range(a, dim)]
    ncell = int(np.prod(ext))
    cells = np.zeros(ncell, dtype=cell_dtype(dim))
    k = idx[:, 0] + ext[0] * (idx[:, 1] + (ext[1] * idx[:, 2] if dim == 3 else 0))
    np.add.at(cells["n"], k, 1)
    for a in range(dim):
        np.add.at(cells["s"][:, a], k, U[:, a])
    for p, (a, b) in enumerate(pairs):
        np.add.at(cells["ss"][:, p], k, U[:, a] * U[:, b])
    o4 = np.zeros((4, 3), dtype=np.float32)
    if dim == 2:
        k0 = [int(np.rint(float(origin[a]) / c)) for a in range(2)]
        for q, (sx, sy) in enumerate(((0.0, 0.0), (0.5, 0.0), (0.0, 0.5), (0.5, 0.5))):
            o4[q, 0] = np.float32((k0[0] - sx) * c)
            o4[q, 1] = np.float32((k0[1] - sy) * c)
    else:
        o4[0] = origin
    h = dict(magic=MAGIC, version=1, dims=dim, ngrid=1, width=ext[0], height=ext[1], depth=ext[2] if dim == 3 else 1,
             cell_bytes=cell_dtype(dim).itemsize, cell_size=float(c), n_cells=ncell, n_points=len(pts) if dim == 2 else 0,
             origin=o4)
    return pack(h, cells), idx, fidx


# ---- how far the coarsened sums may lie from a direct binning of the same points at cell f c ----------------------------
def sum_bounds(n, f):
    """(first sums, off-diagonal second sums, diagonal second sums): the largest |coarsened - direct| for a cell of n points.

    In parent units (c_parent 2^-22) let x be a point's true coordinate from the parent's centre.  The direct binning
    keeps u = rint(x) = x + delta, |delta| <= 1/2.  The fine binning keeps U = rint(f x - Delta) in fine units, and
    coarsening moves it back: v = (U + Delta) / f = x + eps, |eps| <= 1 / (2 f), exactly (N_a = f sum v, N_ab = f^2 sum
    v_a v_b).  So per point |v - u| <= G = 1/2 + 1/(2f) = (f + 1) / (2 f), and with the one rounding to the parent's unit
        |S'_a - S_a|  <= n G + 1/2.
    Second sums: v_a v_b - u_a u_b = u_a g_b + u_b g_a + g_a g_b with |g| <= G and |u| <= 2^21 (a point lies in its cell),
    so per point at most 2^22 G + G^2, and with the one rounding
        |SS'_ab - SS_ab| <= n (2^22 G + G^2) + 1/2.
    A diagonal sum may have been raised to ceil(S'_a^2 / n) (the degenerate-cell clamp).  Then either the direct sum lies
    above it, and the raise only brought SS' closer, or SS_aa >= S_a^2 / n (Cauchy-Schwarz) gives
        SS'_aa - SS_aa <= (S'_a^2 - S_a^2) / n + 1 <= (n G + 1/2)(2^22 n + n G + 1/2) / n + 1
                       <= n (2^22 G + G^2) + 2^21 + G + 2,
    which is the bound used for diagonals."""
    from fractions import Fraction as Fr
    G = Fr(f + 1, 2 * f)
    b1 = n * G + Fr(1, 2)
    b2 = n * ((1 << 22) * G + G * G) + Fr(1, 2)
    return b1, b2, n * ((1 << 22) * G + G * G) + (1 << 21) + G + 2


def check_against_direct(coarse_blob, direct_blob, f):
    """Geometry identical, n equal cell by cell, sums within sum_bounds; returns the largest differences seen."""
    hc, cc = parse(coarse_blob)
    hd, cd = parse(direct_blob)
    for k in ("dims", "ngrid", "width", "height", "depth", "cell_size", "n_cells"):
        assert hc[k] == hd[k], (k, hc[k], hd[k])
    assert np.array_equal(hc["origin"], hd["origin"]), (hc["origin"], hd["origin"])
    assert np.array_equal(cc["n"], cd["n"])
    dim = hc["dims"]
    diag = [p for p, (a, b) in enumerate((a, b) for a in range(dim) for b in range(a, dim)) if a == b]
    worst = [0, 0]
    for k in np.flatnonzero(cc["n"]):
        b1, b2, b2d = sum_bounds(int(cc["n"][k]), f)
        for a in range(dim):
            e = abs(int(cc["s"][k][a]) - int(cd["s"][k][a]))
            assert e <= b1, (k, a, e, b1)
            worst[0] = max(worst[0], e)
        for p in range(len(cc["ss"][k])):
            e = abs(int(cc["ss"][k][p]) - int(cd["ss"][k][p]))
            assert e <= (b2d if p in diag else b2), (k, p, e)
            worst[1] = max(worst[1], e)
    return worst
