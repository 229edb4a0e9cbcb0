"""CPU: the references of the detection training kernels (tests/ref_det_train.py) on hand-worked cases -- what the GPU tests compare
the kernels against has to be right by itself."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_detection as RD  # noqa: E402
import ref_det_train as RT  # noqa: E402

F32 = np.float32


def test_match_ref_tie_goes_to_the_lower_index():
    # two identical gt boxes: every candidate is tied between them
    gt = np.array([[0, 0, 2, 2], [0, 0, 2, 2], [10, 10, 12, 12]], dtype=F32)
    cand = np.array([[0, 0, 2, 1], [10, 10, 12, 12]], dtype=F32)
    m, best, _, tied = RT.match_ref(gt, cand, 0.3, 0.7, False)
    assert m.tolist() == [-2, 2] and best.tolist() == [0.5, 1.0] and tied.tolist() == [True, False]
    m, _, _, _ = RT.match_ref(gt, cand, 0.3, 0.5, False)
    assert m.tolist() == [0, 2]                      # the lower of the tied indices 0 and 1


def test_match_ref_low_quality_restores_the_candidates_own_argmax():
    # candidate 0 overlaps gt 0 by 1/2 and gt 1 by 1/4; gt 1's best candidate is candidate 0 (candidate 1 has 1/8), gt 0's best is
    # candidate 1 (IoU 1).  With the rule on, candidate 0 -- below the threshold -- is restored, to ITS argmax gt 0, not to gt 1.
    gt = np.array([[0, 0, 4, 4], [3, 0, 4, 2]], dtype=F32)       # gt 1: area 2, inside candidate 0 (area 8) and candidate 1 (area 16)
    cand = np.array([[0, 0, 4, 2], [0, 0, 4, 4], [50, 50, 60, 60]], dtype=F32)
    assert RT.iou_row(gt[0], cand).tolist() == [0.5, 1.0, 0.0] and RT.iou_row(gt[1], cand).tolist() == [0.25, 0.125, 0.0]
    off, _, _, _ = RT.match_ref(gt, cand, 0.6, 0.7, False)
    on, best, restored, _ = RT.match_ref(gt, cand, 0.6, 0.7, True)
    assert off.tolist() == [-1, 0, -1] and best.tolist() == [0.5, 1.0, 0.0]
    assert restored.tolist() == [True, True, False] and on.tolist() == [0, 0, -1]


def test_match_ref_zero_maximum_still_restores():
    # gt 1 overlaps no candidate: its maximum is exactly 0 and every candidate with IoU 0 to it is restored (torchvision's behaviour)
    gt = np.array([[0, 0, 4, 4], [100, 100, 104, 104]], dtype=F32)
    cand = np.array([[0, 0, 4, 2], [50, 50, 60, 60]], dtype=F32)
    on, _, restored, _ = RT.match_ref(gt, cand, 0.6, 0.7, True)
    assert restored.tolist() == [True, True] and on.tolist() == [0, 0]


def test_match_ref_thresholds_hit_exactly():
    # IoU exactly 1/2 ([0,0,2,2] / [0,0,2,1]) and exactly 7/10 (7 x 10 inside 10 x 10): `< low` is below, `>= low and < high` between
    gt = np.array([[0, 0, 2, 2], [64, 0, 74, 10]], dtype=F32)
    cand = np.array([[0, 0, 2, 1], [64, 0, 71, 10]], dtype=F32)
    _, best, _, _ = RT.match_ref(gt, cand, 0.5, 0.7, False)
    assert best[0] == F32(0.5) and best[1] == F32(7.0) / F32(10.0) == F32(0.7)
    assert RT.match_ref(gt, cand, 0.5, 0.7, False)[0].tolist() == [-2, 1]        # exactly low: between; exactly high: matched
    assert RT.match_ref(gt, cand, 0.5, 0.5, False)[0].tolist() == [0, 1]
    assert RT.match_ref(gt, cand, 0.7, 0.7, False)[0].tolist() == [-1, 1]
    assert RT.match_ref(gt, cand, np.nextafter(F32(0.7), F32(1)), 0.9, False)[0].tolist() == [-1, -1]


def test_match_ref_without_gt_boxes():
    m, best, restored, _ = RT.match_ref(np.zeros((0, 4), dtype=F32), np.array([[0, 0, 1, 1]] * 3, dtype=F32), 0.3, 0.7, True)
    assert m.tolist() == [-1, -1, -1] and best.tolist() == [0.0, 0.0, 0.0] and not restored.any()


def test_match_ref_degenerate_pair():
    # a zero-area gt box against a zero-area candidate at the same place: 0 / 0 = NaN, never the maximum
    gt = np.array([[5, 5, 5, 5], [0, 0, 2, 2]], dtype=F32)
    cand = np.array([[5, 5, 5, 5], [0, 0, 2, 2]], dtype=F32)
    assert np.isnan(RT.iou_row(gt[0], cand)[0])
    m, best, restored, _ = RT.match_ref(gt, cand, 0.3, 0.7, True)
    # candidate 0: the NaN is skipped, IoU 0 with gt 1 (index 1, below the threshold).  gt 0's maximum over the candidates is the 0
    # of candidate 1 (its NaN with candidate 0 is left out), which restores candidate 1 alone: a NaN equals nothing.
    assert m.tolist() == [-1, 1] and best.tolist() == [0.0, 1.0] and restored.tolist() == [False, True]
    only, best, restored, _ = RT.match_ref(gt[:1], cand[:1], 0.3, 0.7, True)
    assert only.tolist() == [-1] and best[0] == -np.inf and not restored.any()      # nothing but NaN: index 0, below the threshold


def test_quarter_grid_case_has_ties_and_restored_matches():
    """the GPU test's quarter-grid case is not vacuous"""
    gt, cand = RD.quarter_grid_boxes(12, seed=12)[0], RD.quarter_grid_boxes(500, seed=500)[0]
    on, best, restored, tied = RT.match_ref(gt, cand, 0.5, 0.7, True)
    off = RT.match_ref(gt, cand, 0.5, 0.7, False)[0]
    assert tied.sum() >= 1 and (on != off).sum() >= 1
    assert (best == F32(0.5)).sum() >= 1 and (best == F32(0.7)).sum() >= 1


# ------------------------------------------------------------------------------------------------------------ RoIAlign backward
@pytest.mark.parametrize('K,seed,P,mode', [(1, 11, 7, 'mixed'), (5, 12, 7, 'mixed'), (5, 13, 2, 'mixed'), (4, 14, 7, 'skip'), (3, 15, 2, 'one')])
def test_backward_ref_is_the_adjoint_of_the_forward_ref(K, seed, P, mode):
    """<roi_align_ref(x), g> == <x, backward_ref(g)> to 1e-12 relative, C = 2"""
    feats = RD.roi_features(2, seed=seed)
    rois, levels, _ = RD.roi_cases(K, seed, P, 2, mode)
    rng = np.random.RandomState(seed)
    g = rng.randn(K, 2, P, P)
    fwd = RD.roi_align_ref(feats, RD.SCALES, rois, levels, P, 2)
    grads, cnt, mag = RT.roi_align_backward_ref(g, RD.MAPS, RD.SCALES, rois, levels, 2, P, 2)
    lhs = (fwd * g).sum()
    rhs = sum((np.asarray(f, dtype=np.float64) * d).sum() for f, d in zip(feats, grads))
    scale = sum((np.abs(np.asarray(f, dtype=np.float64)) * m).sum() for f, m in zip(feats, mag))
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), scale)
    for d, c, m in zip(grads, cnt, mag):
        assert np.all(np.abs(d) <= m * (1 + 1e-12)) and np.all((c == 0) == (m.sum(1) == 0))     # the magnitudes bound the gradient


def test_backward_ref_single_sample_by_hand():
    # one RoI of one bin and one sample on a 4 x 4 map, scale 1: box [1, 1, 2.5, 2] -> size max(., 1): 1.5 x 1, sample at
    # x = 1 + 0.75 = 1.75, y = 1 + 0.5 = 1.5: weights (1-.5)(1-.75), (1-.5)(.75), (.5)(1-.75), (.5)(.75) on (1,1) (1,2) (2,1) (2,2)
    rois = np.array([[0, 1, 1, 2.5, 2]], dtype=F32)
    grads, cnt, mag = RT.roi_align_backward_ref(np.full((1, 1, 1, 1), 2.0), [(4, 4)], [1.0], rois, [0], 1, 1, 1)
    want = np.zeros((4, 4))
    want[1, 1], want[1, 2], want[2, 1], want[2, 2] = 0.25, 0.75, 0.25, 0.75
    assert np.allclose(grads[0][0, 0], want, rtol=0, atol=1e-15)
    assert cnt[0][0].sum() == 4 and np.all(mag[0][0, 0][want > 0] == 2.0)
    # a RoI with a level or an image that does not exist contributes nothing
    for bad_rois, bad_levels in ((np.array([[3, 1, 1, 2.5, 2]], dtype=F32), [0]), (rois, [2]), (np.array([[-1, 1, 1, 2.5, 2]], dtype=F32), [0])):
        grads, cnt, _ = RT.roi_align_backward_ref(np.ones((1, 1, 1, 1)), [(4, 4)], [1.0], bad_rois, bad_levels, 1, 1, 1)
        assert not grads[0].any() and not cnt[0].any()
