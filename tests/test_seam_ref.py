"""The exact lookup reference (tests/seam_ref.py) and the seam catalogue (tests/seam_cases.py), checked on the CPU:
the correctly rounded fma against rationals, the pose tie condition (no pose dropped), the seams found on the rule,
both sides of every named seam present, the score terms large against the score tolerance, and a mutant table - every
plausible wrong lookup changes the expected hits of a named catalogue entry."""
import math
from fractions import Fraction

import numpy as np
import pytest

import seam_cases as K
import seam_ref as S

F32 = np.float32


# ------------------------------------------------------------------------------------------------ fma32
def _traps(n, rng):
    """Triples whose exact sum lies 2^-46 relative below a float32 tie of c: the float64 sum rounds ONTO the tie, and a
    second rounding to float32 then goes to the even neighbour - wrong wherever that is not c itself.
    a b = h (1 - 2^-46) with h half an ulp of c: a = 2^e1 (1 + 2^-23), b = 2^e2 (1 - 2^-23)."""
    c = (rng.uniform(1.0, 2.0, n) * 2.0 ** rng.integers(-20, 40, n)).astype(F32)
    h = 0.5 * np.spacing(c).astype(np.float64)
    e = np.log2(h).round().astype(int)
    e1 = e // 2
    a = (np.ldexp(1.0, e1) * (1.0 + 2.0 ** -23)).astype(F32)
    b = (np.ldexp(1.0, e - e1) * (1.0 - 2.0 ** -23)).astype(F32)
    sign = np.where(rng.integers(0, 2, n) > 0, 1.0, -1.0).astype(F32)
    return a * sign, b, c * sign


def test_fma32_is_the_rational_fma():
    rng = np.random.default_rng(20261020)
    n = 100_000
    a = (rng.normal(size=n) * 2.0 ** rng.integers(-12, 12, n)).astype(F32)
    b = (rng.normal(size=n) * 2.0 ** rng.integers(-12, 12, n)).astype(F32)
    c = (rng.normal(size=n) * 2.0 ** rng.integers(-12, 12, n)).astype(F32)
    near = rng.random(n) < 0.5                          # half of them with cancellation: c close to -a b
    c[near] = (-(a[near].astype(np.float64) * b[near]) * (1.0 + rng.normal(0, 1e-4, near.sum()))).astype(F32)
    ta, tb, tc = _traps(2000, rng)
    # true ties: 1 * h + c with h exactly half an ulp of c
    tie_c = (rng.uniform(1.0, 2.0, 500) * 2.0 ** rng.integers(-10, 10, 500)).astype(F32)
    tie_b = (0.5 * np.spacing(tie_c)).astype(F32)
    a, b, c = (np.concatenate(v) for v in ((a, ta, np.ones(500, F32)), (b, tb, tie_b), (c, tc, tie_c)))
    stats = {}
    got = S.fma32(a, b, c, stats)
    want = np.array([S.fma32_fraction(x, y, z) for x, y, z in zip(a, b, c)], F32)
    assert got.tobytes() == want.tobytes()
    old = S.fma32_double_rounded(a, b, c)
    wrong = int((old != want).sum())
    print(f"fma32: {len(a)} triples, {stats['settled']} settled by the error term, {stats['ties']} true ties; "
          f"the double-rounded emulation is wrong on {wrong}")
    assert stats["settled"] >= 1000 and stats["ties"] >= 400 and wrong >= 500
    # scalars and broadcasting
    assert S.fma32(F32(2.0), F32(3.0), F32(1.0)) == F32(7.0)
    assert S.fma32(F32(2.0), np.array([1, 2], F32), F32(1.0)).tolist() == [3.0, 5.0]
    assert np.isnan(S.fma32(F32(np.nan), F32(1.0), F32(1.0)))


def test_round_fraction32_rounds_half_to_even():
    one, up = F32(1.0), np.nextafter(F32(1.0), F32(2.0))
    mid = (Fraction(float(one)) + Fraction(float(up))) / 2
    assert S.round_fraction32(mid) == one                                   # even mantissa
    assert S.round_fraction32(mid + Fraction(1, 2 ** 80)) == up
    up2 = np.nextafter(up, F32(2.0))
    assert S.round_fraction32((Fraction(float(up)) + Fraction(float(up2))) / 2) == up2


# ------------------------------------------------------------------------------------------------ poses
def test_every_pose_keeps_clear_of_float32_rounding_ties():
    dropped = []
    for dim in (2, 3):
        for name, pose in K.POSES[dim].items():
            worst, need = S.pose_margin(pose, dim)
            print(f"{dim}D {name}: nearest tie {worst:.3g} float64 ulps away, needed {need:.3g}")
            if not S.pose_is_tie_free(pose, dim):
                dropped.append((dim, name))
    assert len(dropped) == 0, dropped
    used = {(dim, pn) for dim in (2, 3) for _, _, pn in K.entries(dim)}
    assert used == {(dim, pn) for dim in (2, 3) for pn in K.POSES[dim]}      # and every pose is used
    # the quarter turns: float32(cos) is 6.1e-17, not 0, and goes through the chain as such
    cs, sn, _ = S.rot2d32(math.pi / 2)
    assert 0.0 < float(cs) < 1e-16 and sn == F32(1.0)
    assert any(not -math.pi < K.POSES[2][pn][2] <= math.pi for pn in K.POSES[2])
    assert any(not -math.pi < K.POSES[3][pn][5] <= math.pi for pn in K.POSES[3])


# ------------------------------------------------------------------------------------------------ seams
def test_seam_is_the_first_value_of_its_cell():
    for o, c, k in ((-0.1, 0.1, 1), (799.7, 0.3, 7), (-801.0, 0.75, 3), (0.0, 0.5, 0), (-3.3, 0.3, 11)):
        inv_c = F32(1.0 / c)
        s = S.seam(F32(o), inv_c, k)
        assert S.cell_index32(s, o, inv_c) >= k > S.cell_index32(S.below(s), o, inv_c)


@pytest.mark.parametrize("c", [0.1, 0.3, 0.75])
def test_the_catalogue_tells_the_float32_rule_from_a_float64_division(c):
    """floorf((x - o) * inv_c) in float32 and floor((x - o) / c) in float64 disagree on some catalogue point."""
    differ = total = 0
    for cc, base, pn in K.entries(2):
        if cc != c or pn != "identity":
            continue
        t, src = K.target(2, cc, base), K.source(2, cc, base, pn)
        for a in range(2):
            x = src.coords[a][:src.n_seam_points]
            rule = S.cell_index32(x, t.origin[a], t.grid.inv_c)
            division = np.floor((x.astype(np.float64) - float(t.origin[a])) / c)
            differ += int((rule != division).sum())
            total += len(x)
    print(f"c = {c}: {differ} of {total} seam coordinates lie in another cell under the float64 division")
    assert differ > 0


@pytest.mark.parametrize("dim", [2, 3])
def test_every_entry_has_points_on_both_sides_of_its_seams(dim):
    for c, base, pn in K.entries(dim):
        t, src, pose = K.target(dim, c, base), K.source(dim, c, base, pn), K.POSES[dim][pn]
        img = K.image(dim, src.coords, pose)
        n_named = 0
        for a in range(dim):
            f = S.cell_index32(img[a], t.origin[a], t.grid.inv_c)
            placed = src.seam[:, a] >= 0
            # a placed point is in cell k when on the seam, in cell k - 1 one ulp below it: on the exact image
            assert np.array_equal(f[placed], (src.seam[placed, a] - 1 + src.on[placed, a]).astype(np.float64)), (c, base, pn, a)
            on = set(src.seam[placed & (src.on[:, a] == 1), a].tolist())
            under = set(src.seam[placed & (src.on[:, a] == 0), a].tolist())
            named = on & under                                   # the seams the entry names: both sides are there
            interior = set(range(1, K.SIDE[dim] + 2))
            # at the identity every seam.  Elsewhere a seam value may have no float32 preimage: where the source's ulp is
            # the coarser one (x = 1 - 2^-24 for the image 0.5 - 2^-25 at t = -0.5 does not exist), x + t steps over it;
            # the search keeps what exists, and every axis keeps at least two seams with both sides
            need = len(interior) if pn == "identity" else 2
            assert len(named & interior) >= need, (c, base, pn, a, sorted(named))
            assert {0, t.ext[a]} <= named or pn != "identity", (c, base, pn, a)   # the grid's first and last seam
            n_named += len(named)
        assert n_named >= dim * 6
        assert not S.finite_points(*src.coords)[src.n_seam_points:].all()         # and the non-finite points are there


def test_smallest_score_term_is_a_hundred_tolerances():
    """The score-only families (score_poses, the search volumes) are held to |err| <= 1e-4 |ref| + 1e-3: on the sources
    they are given, one wrong cell moves the score by at least 100 times that."""
    worst = math.inf
    for dim in (2, 3):
        for c, base, pn in K.entries(dim):
            t, src, pose = K.target(dim, c, base), K.source(dim, c, base, pn), K.POSES[dim][pn]
            packs = K.score_packs(t, src, pose, n_packs=3)
            assert len(packs) == 3 and all(len(cc[0]) == K.SCORE_PACK for cc, _, _ in packs)
            for _, score, smallest in packs:
                worst = min(worst, smallest / K.score_tolerance(score))
    print(f"smallest term / tolerance over the catalogue: {worst:.1f}")
    assert worst >= 100.0


def test_build_targets_put_a_point_on_each_side_of_a_cell_seam():
    """The min_points-exact targets: cells with exactly min_points points (valid) and cells that lost their seam point to
    the empty neighbour (min_points - 1: invalid, the neighbour holds 1)."""
    for dim, targets in ((2, K.TARGETS_2D), (3, K.TARGETS_3D)):
        for c, base in targets:
            t = K.target(dim, c, base, True)
            mp = K.MIN_POINTS[dim]
            n = t.grid.count
            assert (n == mp).sum() > 10 and (n == mp - 1).sum() > 5 and (n == 1).sum() == (n == mp - 1).sum(), (t.name, np.bincount(n))
            assert t.grid.n_valid == (n == mp).sum()


# ------------------------------------------------------------------------------------------------ the mutant table
# mutant -> (dimension, entry that catches it, how the reference is evaluated, how the mutant is)
MUTANTS = {
    "(x - o) / c instead of (x - o) * inv_c": (2, (0.3, 0.0, "identity"), {}, dict(index_rule="divide")),
    "the same at c = 0.1, a quarter turn": (2, (0.1, 0.0, "quarter"), {}, dict(index_rule="divide")),
    "the same in 3D at c = 0.75": (3, (0.75, -3.1, "steep"), {}, dict(index_rule="divide")),
    "truncation instead of floor (f in (-1, 0) becomes voxel 0)": (3, (0.5, 0.0, "identity"), dict(neighbourhood=7),
                                                                  dict(neighbourhood=7, index_rule="truncate")),
    "<= at the upper edge (f == extent becomes the last voxel)": (3, (0.5, 0.0, "shift"), dict(neighbourhood=7),
                                                                 dict(neighbourhood=7, index_rule="upper_inclusive")),
    "k_batch3's y + t image in a chain kernel": (3, (1.0, 300.0, "generic_b"), {}, dict(family="batch3")),
    "the chain image in k_batch3": (3, (0.75, -3.1, "steep"), dict(family="batch3"), {}),
    "a float64 image, 2D": (2, (0.1, 800.0, "generic_b"), {}, dict(image_fn=S.image2d_float64)),
    "a float64 image, 3D": (3, (1.0, 300.0, "generic_a"), {}, dict(image_fn=S.image3d_float64)),
}


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_changes_the_expected_hits_of_a_named_entry(mutant):
    dim, (c, base, pn), how_ref, how_mutant = MUTANTS[mutant]
    assert (c, base, pn) in K.entries(dim)
    t, src, pose = K.target(dim, c, base), K.source(dim, c, base, pn), K.POSES[dim][pn]
    ref, mut = K.n_hit(t, src.coords, pose, **how_ref), K.n_hit(t, src.coords, pose, **how_mutant)
    print(f"{mutant}: caught by {K.entry_name(dim, c, base, pn)}: {ref} hits, the mutant {mut}")
    assert ref != mut


def test_mutant_key_arithmetic_at_a_row_end():
    """key + 1 from the last voxel of a row is the first voxel of the next row, key - 1 from the first the last of the row
    before.  With an empty outer ring (every set_target grid) that goes unnoticed, so this entry fills the ring."""
    t, _, src = K.ring_case()
    zero = (0.0,) * 6
    ref = K.n_hit(t, src, zero, neighbourhood=7)
    mut = K.n_hit(t, src, zero, neighbourhood=7, neighbours_by_key=True)
    print(f"key +- 1 at a row end: caught by {K.RING_NAME}: {ref} hits, the mutant {mut}")
    assert ref != mut and K.n_hit(t, src, zero) > 0
    W, H, D = t.grid.dims
    ring = np.zeros((D, H, W), bool)
    ring[:, :, 0] = ring[:, :, -1] = True
    assert (t.grid.valid.reshape(D, H, W) & ring).sum() > 20


def test_truncation_cannot_show_in_2d():
    """In 2D the index is clamped onto a ring that holds no valid cell: f in (-1, 0) truncated to cell 0 and f == extent
    clamped to the last cell both read an invalid cell, as the rule's "outside" does.  Said here so that the mutant table
    does not claim more than it shows."""
    for c, base, pn in K.entries(2)[:8]:
        t, src, pose = K.target(2, c, base), K.source(2, c, base, pn), K.POSES[2][pn]
        ref = K.n_hit(t, src.coords, pose)
        assert ref == K.n_hit(t, src.coords, pose, index_rule="truncate") == K.n_hit(t, src.coords, pose, index_rule="upper_inclusive")
        ring = np.ones((t.grid.H, t.grid.W), bool)
        ring[1:-1, 1:-1] = False
        assert not (t.grid.valid.reshape(t.grid.H, t.grid.W) & ring).any()
