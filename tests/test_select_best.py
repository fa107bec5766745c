"""search.select_best, the numpy restatement of ndt2d/ndt3d_best_poses_dev's selection rule: the cases the GPU tests
then hold the library to."""
import math

import numpy as np
import pytest

from gtsam_ndt_amd import search


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def test_order_is_score_descending_then_index_ascending():
    poses = np.array([[float(i), 0.0, 0.0] for i in range(6)])
    hits = search.select_best(_f32([1.0, 3.0, 3.0, 0.5, 3.0, 2.0]), poses, k=6, min_sep=(0.0, 0.0))
    assert [h.index for h in hits] == [1, 2, 4, 5, 0, 3]
    assert [h.score for h in hits] == [3.0, 3.0, 3.0, 2.0, 1.0, 0.5]
    assert hits[0].pose == (1.0, 0.0, 0.0)


def test_duplicates_stay_at_zero_separation_and_go_at_any_positive_one():
    poses = np.array([[1.0, 2.0, 0.3]] * 3 + [[5.0, 5.0, 0.0]])
    s = _f32([2.0, 2.0, 1.0, 0.5])
    assert [h.index for h in search.select_best(s, poses, 8, (0.0, 0.0))] == [0, 1, 2, 3]
    assert [h.index for h in search.select_best(s, poses, 8, (1e-9, 1e-9))] == [0, 3]


def test_a_pose_is_dropped_only_when_close_in_translation_and_in_rotation():
    poses = np.array([[0.0, 0.0, 0.0],
                      [0.1, 0.0, 1.0],        # close in translation only
                      [3.0, 0.0, 0.01],       # close in rotation only
                      [0.1, 0.1, 0.01],       # close in both: dropped
                      [0.5, 0.0, 0.0],        # exactly 0.5 away: the comparison is strict, kept
                      [0.0, 0.0, 0.1]])       # exactly 0.1 in rotation: kept
    hits = search.select_best(_f32([6, 5, 4, 3, 2, 1]), poses, 8, (0.5, 0.1))
    assert [h.index for h in hits] == [0, 1, 2, 4, 5]


def test_the_heading_difference_is_wrapped_and_the_poses_are_not():
    poses = np.array([[0.0, 0.0, math.pi - 0.01], [0.0, 0.0, -math.pi + 0.01], [0.0, 0.0, 3.0 * math.pi - 0.01]])
    hits = search.select_best(_f32([3, 2, 1]), poses, 8, (0.5, 0.1))
    assert [h.index for h in hits] == [0]
    hits = search.select_best(_f32([1, 2, 3]), poses, 8, (0.5, 0.001))
    assert [h.index for h in hits] == [2, 1] and hits[0].pose[2] == 3.0 * math.pi - 0.01


def test_the_3d_measures_take_z_and_the_largest_angle():
    base = [1.0, 2.0, 3.0, 0.1, 0.2, 0.3]
    poses = np.array([base,
                      [1.0, 2.0, 3.6, 0.1, 0.2, 0.3],       # 0.6 away in z alone: kept
                      [1.0, 2.0, 3.0, 0.1, 0.35, 0.3],      # pitch 0.15 away: kept
                      [1.2, 2.2, 3.2, 0.15, 0.25, 0.35],    # 0.35 m and 0.05 rad away: dropped
                      [1.0, 2.0, 3.0, 0.1 + 2.0 * math.pi, 0.2, 0.3 - 2.0 * math.pi]])   # the same rotation: dropped
    hits = search.select_best(_f32([5, 4, 3, 2, 1]), poses, 8, (0.5, 0.1))
    assert [h.index for h in hits] == [0, 1, 2]
    assert len(hits[0].pose) == 6


def test_the_shortlist_holds_the_best_4096_candidates():
    """5000 candidates in one spot and a lone one elsewhere that ranks 4500th: beyond the shortlist, it is never
    reached, whereas among 4000 it is."""
    n = 5000
    poses = np.zeros((n, 3))
    scores = np.linspace(2.0, 1.0, n).astype(np.float32)
    poses[4500] = (50.0, 50.0, 0.0)
    assert [h.index for h in search.select_best(scores, poses, 8, (1.0, 1.0))] == [0]
    poses[4500] = 0.0
    poses[4000] = (50.0, 50.0, 0.0)
    assert [h.index for h in search.select_best(scores, poses, 8, (1.0, 1.0))] == [0, 4000]


def test_k_larger_than_the_survivors_and_a_list_without_a_positive_score():
    poses = np.array([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0], [0.1, 0.0, 0.0]])
    assert [h.index for h in search.select_best(_f32([1, 2, 3]), poses, 64, (0.5, 0.1))] == [2, 1]
    assert [h.index for h in search.select_best(_f32([1, 2, 3]), poses, 1, (0.5, 0.1))] == [2]
    assert search.select_best(_f32([0, 0, 0]), poses, 8) == []
    assert search.select_best(_f32([0.0, -0.0, 0.0]), poses, 8, (0.0, 0.0)) == []
    with pytest.raises(ValueError):
        search.select_best(_f32([1, 2]), poses, 8)
