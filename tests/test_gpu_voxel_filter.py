"""ndt2d/ndt3d_voxel_filter* on the device (docs/ALGORITHM.md section 2.24) against the exact reference
tests/voxel_filter_ref.py - counts, order and info exactly, every coordinate within 1/2 ulp32(X) + 2 eps64 (|centre| +
leaf) of the exact centroid X - and, bit for bit, against the numpy restatement gtsam_ndt_amd/voxel.py.  Shapes are the
smallest that reach every seam of csrc/ndt_voxel_filter.hpp: bitmap word edges (32 voxels), the rank passes' chunk
(kVoxChunk = 2048 words = 65536 voxels), the single-workgroup scan's trip (256 chunks), the emit tile (256 voxels)."""
import ctypes as C
import functools
import os
import time

import numpy as np
import pytest

import voxel_filter_ref as R
from gtsam_ndt_amd import voxel

pytestmark = pytest.mark.gpu

CHUNK_VOXELS = 2048 * 32
SLEEP_CYCLES = 50_000_000                      # some 25 ms of torch.cuda._sleep on the producer stream
CANARY = -777.0


def _cloud(dim, n, seed, span=4.0):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-span, span, (n, dim)).astype(np.float32)
    p[::5] = np.round(p[::5] * 4.0) / 4.0      # every fifth point on planes of the 0.25 lattice
    return p


@functools.lru_cache(maxsize=None)
def _case(dim, n, seed, leaf, min_points=1, span=4.0):
    pts = _cloud(dim, n, seed, span)
    pts.setflags(write=False)
    return pts, R.reference(pts, leaf, min_points)


def _matcher(dim):
    from gtsam_ndt_amd.matcher import NdtMatcher2D, NdtMatcher3D
    return NdtMatcher2D() if dim == 2 else NdtMatcher3D()


def _dev(pts):
    import torch
    return tuple(torch.from_numpy(np.array(pts[:, k], dtype=np.float32)).cuda() for k in range(pts.shape[1]))      # (a writable copy)


def _run(m, pts, leaf, min_points=1):
    """The matcher's call on a device copy of pts -> (points [m, dim] float32, counts, (n_invalid, n_voxels, n_out))."""
    out, cnt, info = m.voxel_filter(*_dev(pts), leaf, min_points, with_counts=True, with_info=True)
    p = np.stack([o.cpu().numpy() for o in out], axis=1) if info.n_out else np.zeros((0, pts.shape[1]), np.float32)
    return p, cnt.cpu().numpy(), (info.n_invalid, info.n_voxels, info.n_out)


def _same_as_numpy(got, pts, leaf, min_points=1):
    wp, wc, wi = voxel.voxel_filter(pts, leaf, min_points, with_info=True)
    assert got[2] == (wi["n_invalid"], wi["n_voxels"], wi["n_out"])
    assert np.array_equal(got[1], wc)
    assert got[0].tobytes() == wp.tobytes(), "the device's mu differs from the written contract"


def _raw(m, dcoords, leaf, min_points, out, cnt, capacity, n=None):
    """ndt*_voxel_filter_dev as the C ABI has it, into the caller's tensors -> (status, info triple, message)."""
    from gtsam_ndt_amd import _lib as L
    info = L.VoxelFilterInfo()
    ptr = lambda t: None if t is None else t.data_ptr()
    m.wait_stream()
    st = m._c.voxel_filter_dev(m._h, *[ptr(c) for c in dcoords], dcoords[0].numel() if n is None else n, float(leaf), int(min_points),
                               *[ptr(o) for o in out], ptr(cnt), int(capacity), C.byref(info))
    return st, (int(info.n_invalid), int(info.n_voxels), int(info.n_out)), m._lib.ndt_last_error().decode()


# ------------------------------------------------------------------------------------------------ the contract
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("leaf", [0.25, 0.3])
@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_bit_for_bit_against_the_contract(gpu_lib, dim, leaf, n):
    pts, ref = _case(dim, n, 100 * dim + n % 97, leaf)
    with _matcher(dim) as m:
        got = _run(m, pts, leaf)
    worst = R.check(*got, ref, leaf)
    print(f"dim {dim} leaf {leaf} n {n}: {got[2][2]} voxels, worst error / bound {worst:.3f}")
    _same_as_numpy(got, pts, leaf)


# ------------------------------------------------------------------------------------------------ seams
def _at(voxels, leaf, dim, jitter_seed=0, per_voxel=2):
    """Points inside the voxels (rows of lattice indices): per_voxel points each, away from the planes."""
    rng = np.random.default_rng(jitter_seed)
    v = np.repeat(np.asarray(voxels, dtype=np.float64), per_voxel, axis=0)
    return ((v + rng.uniform(0.2, 0.8, v.shape)) * leaf).astype(np.float32)[:, :dim]


@pytest.mark.parametrize("leaf", [0.25, 0.3])
def test_bitmap_word_edges(gpu_lib, leaf):
    """A box of 96 x 3: x-indices 31 | 32 and 63 | 64 of every row are word edges, and so are the rows' ends."""
    vox = [(ix, iy) for iy in (-1, 0, 1) for ix in (-40, -10, -9, -8, -7, 22, 23, 24, 25, 55)]      # box x = -40 .. 55
    pts = _at(vox, leaf, 2, 1)
    ref = R.reference(pts, leaf)
    assert [k for k in ref["keys"]] == sorted(vox, key=lambda t: t[::-1])
    with _matcher(2) as m:
        got = _run(m, pts, leaf)
    R.check(*got, ref, leaf)
    _same_as_numpy(got, pts, leaf)


@pytest.mark.parametrize("dim", [2, 3])
def test_more_occupied_words_than_a_scan_chunk(gpu_lib, dim):
    """A box of 300 x 500 (2D) or 60 x 50 x 50 (3D) voxels = 2.3 chunks of the rank passes, some 3000 occupied words, and
    occupied voxels on both sides of the first chunk edge (box indices 65535 | 65536)."""
    leaf = 0.25
    ext = (300, 500) if dim == 2 else (60, 50, 50)
    rng = np.random.default_rng(9)
    inside = np.stack([rng.integers(0, e, 7000) for e in ext], axis=1)
    edge = []
    for lin in (0, CHUNK_VOXELS - 1, CHUNK_VOXELS, 2 * CHUNK_VOXELS - 1, 2 * CHUNK_VOXELS, int(np.prod(ext)) - 1):
        idx, rest = [], lin
        for e in ext:
            idx.append(rest % e)
            rest //= e
        edge.append(idx)
    vox = np.concatenate([inside, np.array(edge)]) - 17                      # the box starts at -17 on every axis
    pts = _at(vox, leaf, dim, 2, per_voxel=1)
    ref = R.reference(pts, leaf)
    words = {(((k[-1] + 17) * ext[1] + (k[1] + 17)) * ext[0] + (k[0] + 17) if dim == 3 else (k[1] + 17) * ext[0] + (k[0] + 17)) >> 5
             for k in ref["keys"]}
    assert len(words) > 2048 and {CHUNK_VOXELS // 32 - 1, CHUNK_VOXELS // 32} <= words
    with _matcher(dim) as m:
        got = _run(m, pts, leaf)
    R.check(*got, ref, leaf)
    _same_as_numpy(got, pts, leaf)


@pytest.mark.parametrize("dim", [2, 3])
def test_a_box_of_one_voxel(gpu_lib, dim):
    pts = _at([(-3, 7, 2)] * 300, 0.3, dim, 3)
    ref = R.reference(pts, 0.3)
    with _matcher(dim) as m:
        got = _run(m, pts, 0.3)
    assert got[2] == (0, 1, 1) and list(got[1]) == [600]
    R.check(*got, ref, 0.3)
    _same_as_numpy(got, pts, 0.3)


@pytest.mark.parametrize("dim", [2, 3])
def test_a_box_of_two_to_the_thirty_with_two_occupied_corners(gpu_lib, dim):
    """The largest box the call takes, 2^30 voxels (2^25 bitmap words, 2^14 chunks, 64 trips of the scan), and the first
    one it refuses."""
    leaf = 0.25
    ext = (32768, 32768) if dim == 2 else (1024, 1024, 1024)
    lo = tuple(-(e // 2) for e in ext)
    hi = tuple(l + e - 1 for l, e in zip(lo, ext))
    pts = _at([lo, hi, hi], leaf, dim, 4, per_voxel=1)
    ref = R.reference(pts, leaf)
    from gtsam_ndt_amd import _lib as L
    with _matcher(dim) as m:
        _run(m, pts[:1], leaf)                                   # (the first call of a handle allocates its header)
        t0 = time.perf_counter()
        got = _run(m, pts, leaf)
        dt = time.perf_counter() - t0
        print(f"{dim}D box of 2^30 voxels: {dt * 1e3:.1f} ms")
        assert got[2] == (0, 2, 2) and list(got[1]) == [1, 2]
        R.check(*got, ref, leaf)
        _same_as_numpy(got, pts, leaf)
        # one voxel more along x
        over = np.concatenate([pts, _at([(hi[0] + 1,) + hi[1:]], leaf, dim, 5, per_voxel=1)])
        import torch
        d = _dev(over)
        out = [torch.full((4,), CANARY, dtype=torch.float32, device="cuda") for _ in range(dim)]
        st, info, msg = _raw(m, d, leaf, 1, out, None, 4)
        assert st == L.NDT_ERR_CAPACITY and "2^30" in msg and "voxel_filter_dev" in msg, (st, msg)
        assert info == (0, 0, 0) and all((o.cpu().numpy() == CANARY).all() for o in out)
        got = _run(m, pts, leaf)                                 # the handle is as good as before
        assert got[2] == (0, 2, 2)


# ------------------------------------------------------------------------------------------------ permutation
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("min_points", [1, 2])
def test_every_order_of_the_input_gives_the_same_bits(gpu_lib, dim, min_points):
    pts = _cloud(dim, 4099, 31 + dim, span=3.0).copy()
    pts[11, 0], pts[1234, dim - 1] = np.nan, np.inf
    with _matcher(dim) as m:
        want = _run(m, pts, 0.3, min_points)
        assert want[2][0] == 2 and 0 < want[2][2] <= want[2][1] < 4097
        for seed in (1, 2, 3):
            got = _run(m, np.random.default_rng(seed).permutation(pts), 0.3, min_points)
            assert got[2] == want[2] and got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    _same_as_numpy(want, pts, 0.3, min_points)


# ------------------------------------------------------------------------------------------------ min_points
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("min_points", [2, 3])
def test_min_points_drops_thin_voxels_and_keeps_the_order(gpu_lib, dim, min_points):
    """4099 points over some 1000 (2D) or 4000 (3D) voxels: more than one emit tile, voxels of one to a dozen points."""
    span = 4.0 if dim == 2 else 2.0
    pts, ref = _case(dim, 4099, 55 + dim, 0.25, min_points, span)
    _, ref1 = _case(dim, 4099, 55 + dim, 0.25, 1, span)
    with _matcher(dim) as m:
        got = _run(m, pts, 0.25, min_points)
    assert got[2][1] == ref1["info"][1] and got[2][2] == ref["info"][2] and 256 < got[2][2] < got[2][1]
    assert int(got[1].min()) >= min_points
    R.check(*got, ref, 0.25)                                      # counts, and through the coordinates the order
    _same_as_numpy(got, pts, 0.25, min_points)


# ------------------------------------------------------------------------------------------------ invalid points
@pytest.mark.parametrize("dim", [2, 3])
def test_invalid_points_are_counted_and_never_come_out(gpu_lib, dim):
    leaf = 0.25
    pts = _cloud(dim, 1500, 77, span=3.0).copy()
    edge = np.float32(2.0 ** 30 * leaf)
    bad = {3: np.nan, 300: np.inf, 301: -np.inf, 777: edge, 1000: -edge, 1499: np.float32(3e38)}
    for j, (i, v) in enumerate(bad.items()):
        pts[i, j % dim] = v
    ref = R.reference(pts, leaf)
    assert ref["info"][0] == len(bad)
    with _matcher(dim) as m:
        got = _run(m, pts, leaf)
        assert got[2][0] == len(bad) and int(got[1].sum()) == 1500 - len(bad)
        assert np.isfinite(got[0]).all() and np.abs(got[0]).max() < 3.1
        R.check(*got, ref, leaf)
        _same_as_numpy(got, pts, leaf)
        allbad = np.full((300, dim), np.nan, np.float32)
        allbad[7], allbad[8, 0] = np.inf, edge
        for min_points in (1, 2):
            assert _run(m, allbad, leaf, min_points)[2] == (300, 0, 0)          # NDT_OK: the matcher would have raised
        assert _run(m, pts, leaf)[0].tobytes() == got[0].tobytes()


# ------------------------------------------------------------------------------------------------ capacity
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("min_points", [1, 2])
def test_capacity_is_respected_to_the_element(gpu_lib, dim, min_points):
    import torch
    from gtsam_ndt_amd import _lib as L
    pts, ref = _case(dim, 4099, 55 + dim, 0.25, min_points, 4.0 if dim == 2 else 2.0)
    n_out = ref["info"][2]
    d = _dev(pts)
    with _matcher(dim) as m:
        want = _run(m, pts, 0.25, min_points)
        for capacity, status in ((n_out - 1, L.NDT_ERR_CAPACITY), (n_out, 0)):
            out = [torch.full((n_out + 64,), CANARY, dtype=torch.float32, device="cuda") for _ in range(dim)]
            cnt = torch.full((n_out + 64,), 0x7A7A7A7A, dtype=torch.int32, device="cuda")
            st, info, msg = _raw(m, d, 0.25, min_points, out, cnt, capacity)
            assert st == status and info == ref["info"], (capacity, st, info, msg)
            if st:
                assert "n_out" in msg
            for a, o in enumerate(out):
                o = o.cpu().numpy()
                assert (o[capacity:] == CANARY).all()
                assert o[:capacity].tobytes() == want[0][:capacity, a].tobytes()         # what fits is the front of the result
            c = cnt.cpu().numpy()
            assert (c[capacity:] == 0x7A7A7A7A).all() and np.array_equal(c[:capacity], want[1][:capacity].astype(np.int32))
        # the counts are optional
        out = [torch.full((n_out,), CANARY, dtype=torch.float32, device="cuda") for _ in range(dim)]
        st, info, _ = _raw(m, d, 0.25, min_points, out, None, n_out)
        assert st == 0 and np.stack([o.cpu().numpy() for o in out], 1).tobytes() == want[0].tobytes()


def test_outputs_that_overlap_the_inputs_are_refused(gpu_lib):
    import torch
    from gtsam_ndt_amd import _lib as L
    pts, _ = _case(2, 257, 200 + 257 % 97, 0.3)
    d = _dev(pts)
    with _matcher(2) as m:
        fresh = torch.empty(257, dtype=torch.float32, device="cuda")
        st, _, msg = _raw(m, d, 0.3, 1, [fresh, d[0][256:]], None, 1)
        assert st == L.NDT_ERR_INVALID_ARG and "overlaps" in msg
        st, _, msg = _raw(m, d, 0.3, 1, [d[1], fresh], None, 257)
        assert st == L.NDT_ERR_INVALID_ARG and "overlaps" in msg


# ------------------------------------------------------------------------------------------------ the handle
@pytest.mark.parametrize("dim", [2, 3])
def test_no_target_is_needed_and_none_is_disturbed(gpu_lib, dim):
    import point_fit_cases as PC
    fx = PC.fixture(dim)
    src = np.stack(fx["source"], axis=1)[:4096]
    init = (0.0,) * (3 if dim == 2 else 6)
    with _matcher(dim) as bare:
        fresh = _run(bare, src, 0.3)                            # a handle that never saw a target
    with PC.matcher(dim) as m:
        before = m.align(*_dev(src), init)
        blob = np.asarray(m.save_map()).tobytes()
        got = _run(m, src, 0.3)
        assert np.asarray(m.save_map()).tobytes() == blob
        after = m.align(*_dev(src), init)
    assert got[2] == fresh[2] and got[0].tobytes() == fresh[0].tobytes()
    assert after.pose == before.pose and after.score == before.score and after.iterations == before.iterations
    assert np.array_equal(after.H, before.H) and after.n_hit == before.n_hit
    _same_as_numpy(got, src, 0.3)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("fixed", [0, 6])
def test_a_pending_async_alignment_is_finished_not_corrupted(gpu_lib, dim, fixed):
    import point_fit_cases as PC
    fx = PC.fixture(dim)
    src = np.stack(fx["source"], axis=1)[:900 if dim == 2 else 4096]
    d = _dev(src)
    init = (0.0,) * (3 if dim == 2 else 6)
    with PC.matcher(dim, fixed_iterations=fixed) as m:
        want = m.align(*d, init)
        alone = _run(m, src, 0.3)
        m.align_async(*d, init)
        during = _run(m, src, 0.3)
        got = m.finish()
    assert got.pose == want.pose and got.iterations == want.iterations and got.score == want.score
    assert got.status == want.status and got.n_hit == want.n_hit and np.array_equal(got.H, want.H)
    assert during[2] == alone[2] and during[0].tobytes() == alone[0].tobytes()


@pytest.mark.parametrize("dim", [2, 3])
def test_input_written_on_a_late_producer_stream(gpu_lib, dim):
    import torch
    pts, _ = _case(dim, 4099, 100 * dim + 4099 % 97, 0.3)
    d = _dev(pts)
    with _matcher(dim) as m:
        want = _run(m, pts, 0.3)
        junk = [torch.full((4099,), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2 * dim)]
        torch.cuda.synchronize()
        del junk                                                 # NaN in the blocks the next allocations are handed
        producer = torch.cuda.Stream()
        with torch.cuda.stream(producer):
            torch.cuda._sleep(SLEEP_CYCLES)                      # the producer stream is busy ...
            late = tuple(c + 0.0 for c in d)                     # ... so the cloud does not exist yet
            out, info = m.voxel_filter(*late, 0.3, with_info=True)         # wait_stream(producer) inside; no host synchronisation
        assert (info.n_invalid, info.n_voxels, info.n_out) == want[2]
        assert np.stack([o.cpu().numpy() for o in out], axis=1).tobytes() == want[0].tobytes()
        assert m.voxel_filter_info == info


def test_scratch_is_reused_and_grows(gpu_lib):
    """One 3D handle: a large call, a small one in the large one's scratch, then a call that outgrows it (more voxels,
    a larger box, min_points = 2 for the tile arrays) - and a 2D handle the same way."""
    for dim in (3, 2):
        with _matcher(dim) as m:
            for n, leaf, min_points, span in ((4099, 0.25, 1, 4.0), (257, 0.3, 1, 4.0), (255, 0.3, 2, 0.5), (9001, 0.25, 2, 9.0),
                                              (4099, 0.25, 1, 4.0)):
                pts, ref = _case(dim, n, 100 * dim + n % 97, leaf, min_points, span)
                got = _run(m, pts, leaf, min_points)
                R.check(*got, ref, leaf)
                _same_as_numpy(got, pts, leaf, min_points)


def test_host_arrays_in_and_out(gpu_lib):
    for dim in (2, 3):
        pts, ref = _case(dim, 4099, 100 * dim + 4099 % 97, 0.3)
        with _matcher(dim) as m:
            out, cnt, info = m.voxel_filter(*[np.ascontiguousarray(pts[:, k]) for k in range(dim)], 0.3, with_counts=True, with_info=True)
            assert all(isinstance(o, np.ndarray) and o.dtype == np.float32 for o in out)
            got = (np.stack(out, axis=1), cnt, (info.n_invalid, info.n_voxels, info.n_out))
            R.check(*got, ref, 0.3)
            _same_as_numpy(got, pts, 0.3)
            # the C entry with too little room: the error, info filled, nothing written
            from gtsam_ndt_amd import _lib as L
            a = [np.ascontiguousarray(pts[:, k]) for k in range(dim)]
            o = [np.full(8, CANARY, np.float32) for _ in range(dim)]
            fi = L.VoxelFilterInfo()
            st = m._c.voxel_filter(m._h, *[c.ctypes.data for c in a], 4099, 0.3, 1, *[c.ctypes.data for c in o], None, 8, C.byref(fi))
            assert st == L.NDT_ERR_CAPACITY and int(fi.n_out) == ref["info"][2] and all((c == CANARY).all() for c in o)


# ------------------------------------------------------------------------------------------------ end to end
def test_filtered_scan_aligns_like_the_oracle_3d(gpu_lib):
    """The 4096-point 3D fixture's source filtered at leaf = 0.5 (2224 voxels) and aligned from the fixture's start, against
    the float64 oracle's alignment of the REFERENCE-filtered points (the exact centroids rounded to float32) from the same
    start.  Checked on the CPU first: the oracle converges there (status 0, 21 iterations; its float32 mirror ends 2e-7
    from it)."""
    import point_fit_cases as PC
    from oracle import ndt3d as o
    g = np.load(os.path.join(PC.HERE, "golden", "ndt3d_small.npz"))
    src = np.stack([g["sx"], g["sy"], g["sz"]], axis=1)
    init = tuple(float(v) for v in g["init"])
    ref = R.reference(src, 0.5)
    want_pts = np.array([[float(x) for x in row] for row in ref["X"]]).astype(np.float32)
    prm = o.Ndt3Params()
    want = o.align3(o.build_grid3(g["tx"], g["ty"], g["tz"], prm), *(np.ascontiguousarray(want_pts[:, k]) for k in range(3)), init, prm)
    assert want["status"] == 0
    with PC.matcher(3) as m:
        out, info = m.voxel_filter(*_dev(src), 0.5, with_info=True)
        assert info.n_out == len(want_pts) < len(src) and info.n_invalid == 0
        got = m.align(*out, init)
    e = np.abs(np.array(got.pose) - np.array(want["pose"]))
    print(f"{info.n_out} of {len(src)} points; against the oracle {e}")
    assert got.status == 0 and e.max() < 1e-4
