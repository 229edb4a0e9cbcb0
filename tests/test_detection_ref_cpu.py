"""tests/ref_detection.py (the reference the detection kernels are judged against) pinned by hand-computed answers."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ref_detection as RD  # noqa: E402


def test_nms_threshold_is_strict():
    # [0,0,2,2] and [0,0,2,1]: intersection 2, union 4 -> IoU exactly 0.5
    boxes = np.array([[0, 0, 2, 2], [0, 0, 2, 1]], dtype=np.float32)
    assert RD.nms_ref(boxes, [0, 0], 0.5).tolist() == [True, True]          # equal is kept
    assert RD.nms_ref(boxes, [0, 0], 0.49).tolist() == [True, False]


def test_nms_chain_keeps_what_only_a_suppressed_box_overlaps():
    # A = [0,10], B = [4,14], C = [8,18] (height 10): IoU(A,B) = IoU(B,C) = 6/14 > 0.4, IoU(A,C) = 2/18 < 0.4
    boxes = np.array([[0, 0, 10, 10], [4, 0, 14, 10], [8, 0, 18, 10]], dtype=np.float32)
    assert RD.nms_ref(boxes, [0, 0, 0], 0.4).tolist() == [True, False, True]


def test_nms_groups_never_suppress_each_other():
    boxes = np.array([[0, 0, 10, 10]] * 4, dtype=np.float32)
    assert RD.nms_ref(boxes, [0, 1, 0, 1], 0.5).tolist() == [True, True, False, False]
    assert RD.nms_ref(boxes, [0, 1, 2, 3], 0.5).tolist() == [True, True, True, True]


def test_nms_tied_scores_resolve_to_the_lower_index():
    boxes = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [50, 50, 60, 60], [0, 0, 10, 10]], dtype=np.float32)
    scores = np.array([0.5, 0.5, 0.5, 0.9], dtype=np.float32)
    # order: 3 (0.9), then 0, 1, 2 by index; 3 suppresses 0 and 1
    assert RD.batched_nms_ref(boxes, scores, [0, 0, 0, 0], 0.5).tolist() == [3, 2]
    assert RD.batched_nms_ref(boxes[:3], scores[:3], [0, 0, 0], 0.5).tolist() == [0, 2]
    assert RD.nms_ref(np.zeros((0, 4), np.float32), [], 0.5).tolist() == []


def _ramp(C, H, W, a, b):
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    return np.stack([a * y + b * x + c for c in range(C)])[None].astype(np.float64)


def test_roi_align_of_a_constant_map_is_the_constant():
    fm = np.full((1, 3, 9, 11), 2.5)
    rois = np.array([[0, 1.0, 2.0, 7.5, 6.25], [0, 0.0, 0.0, 10.0, 8.0]])
    out = RD.roi_align_ref([fm], [1.0], rois, [0, 0], 7, 2)
    assert out.shape == (2, 3, 7, 7) and np.allclose(out, 2.5, rtol=0, atol=1e-12)


def test_roi_align_of_a_ramp_is_the_ramp_at_the_sample_mean():
    a, b, P, S, scale = 0.75, -1.5, 3, 2, 0.5
    fm = _ramp(2, 12, 16, a, b)
    roi = np.array([0, 4.0, 2.0, 22.0, 17.0])          # map coordinates x 2..11, y 1..8.5: wholly inside
    out = RD.roi_align_ref([fm], [scale], roi[None], [0], P, S)[0]
    bin_h, bin_w = (8.5 - 1.0) / P, (11.0 - 2.0) / P
    for ph in range(P):
        for pw in range(P):
            ym, xm = 1.0 + (ph + 0.5) * bin_h, 2.0 + (pw + 0.5) * bin_w        # the mean of the bin's 2 x 2 samples
            for c in range(2):
                assert abs(out[c, ph, pw] - (a * ym + b * xm + c)) < 1e-12


def test_roi_align_beyond_minus_one_is_zero_and_degenerate_is_size_one():
    fm = _ramp(1, 8, 8, 1.0, 1.0) + 1.0
    far = np.array([[0, -40.0, -40.0, -10.0, -10.0]])
    assert np.all(RD.roi_align_ref([fm], [1.0], far, [0], 2, 2) == 0.0)
    # x2 < x1, y2 < y1: the RoI is 1 x 1 from (x1, y1) -> with P = 1, S = 2 the samples sit at +0.25 and +0.75: mean at +0.5
    deg = np.array([[0, 3.0, 2.0, 1.0, 0.5]])
    out = RD.roi_align_ref([fm], [1.0], deg, [0], 1, 2)
    assert abs(out[0, 0, 0, 0] - ((2.5 + 3.5) + 1.0)) < 1e-12
    ys, xs = RD.roi_samples(deg[0, 1:], 1.0, 1, 2)
    assert ys.tolist() == [2.25, 2.75] and xs.tolist() == [3.25, 3.75]


def test_shared_generators_are_usable():
    """the seeds the GPU tests use: few RoIs lost to the exclusion band, many exact-threshold pairs on the quarter grid"""
    for K, seed in ((1, 11), (37, 12), (300, 13)):
        for P in (7, 2):
            for mode in ('mixed', 'one', 'skip'):
                rois, levels, dropped = RD.roi_cases(K, seed, P, 2, mode)
                assert rois.shape == (K, 5) and dropped <= 0.05 * K, (K, P, mode, dropped)
    boxes, scores, groups = RD.quarter_grid_boxes(129, 5)
    x1, y1, x2, y2 = boxes.T.astype(np.float64)
    area = (x2 - x1) * (y2 - y1)
    w = np.maximum(0, np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]))
    h = np.maximum(0, np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]))
    iou = w * h / (area[:, None] + area[None] - w * h)
    assert (iou == 0.5).sum() >= 50 and (np.abs(iou - 0.7) < 1e-12).sum() >= 50
