"""tests/ref_det_post.py (the restatement the GPU tests of sc2_det_postprocess compare against) pinned without a GPU: on hand-worked
cases, and against the package's own torch-op `RoIHeads.postprocess_detections` on the CPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_det_post as RP  # noqa: E402

F32 = np.float32
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
CLIP = math.log(1000.0 / 16)


def table(rows):
    """rows: per proposal a list of (score, box) per foreground class -> (scores f32 [R,C-1], boxes f32 [R,C-1,4])"""
    return (np.array([[s for s, _ in r] for r in rows], dtype=F32), np.array([[b for _, b in r] for r in rows], dtype=F32))


def test_chain_the_suppressed_middle_box_suppresses_nothing():
    """A, B, C shifted by 2 along x, 10 x 10: IoU(A, B) = IoU(B, C) = 8 / 12 > 0.5, IoU(A, C) = 6 / 14 < 0.5 -> A and C stay"""
    s, b = table([[(0.9, [0, 0, 10, 10])], [(0.8, [2, 0, 12, 10])], [(0.7, [4, 0, 14, 10])]])
    (boxes, scores, labels), = RP.stage_b_ref(s, b, [3], 0.05, 0.01, 0.5, 100)
    assert scores.tolist() == [F32(0.9), F32(0.7)] and labels.tolist() == [1, 1]
    assert boxes.tolist() == [[0, 0, 10, 10], [4, 0, 14, 10]]
    # ... and at a threshold above 8 / 12 all three stay, in score order
    (_, scores, _), = RP.stage_b_ref(s, b, [3], 0.05, 0.01, 0.7, 100)
    assert scores.tolist() == [F32(0.9), F32(0.8), F32(0.7)]


def test_equal_scores_go_by_flat_index_and_classes_do_not_meet():
    """three candidates of one score: (row 0, class 1), (row 0, class 2), (row 1, class 1) is the order of their flat indices; the
    two boxes of row 0 are the same box in two classes and both stay; a higher score of a later flat index still comes first"""
    same = [0, 0, 10, 10]
    s, b = table([[(0.5, same), (0.5, same)], [(0.5, [50, 50, 60, 60]), (0.75, [80, 80, 90, 90])]])
    (boxes, scores, labels), = RP.stage_b_ref(s, b, [2], 0.05, 0.01, 0.5, 100)
    assert labels.tolist() == [2, 1, 2, 1] and scores.tolist() == [0.75, 0.5, 0.5, 0.5]
    assert boxes.tolist() == [[80, 80, 90, 90], same, same, [50, 50, 60, 60]]
    # identical boxes of ONE class: the lower flat index stays, its copy goes
    s, b = table([[(0.5, same)], [(0.5, same)]])
    (boxes, scores, labels), = RP.stage_b_ref(s, b, [2], 0.05, 0.01, 0.5, 100)
    assert labels.tolist() == [1] and boxes.tolist() == [same]


def test_truncation_at_d_comes_after_the_suppression():
    rows = [[(0.9 - 0.1 * i, [20.0 * i, 0, 20.0 * i + 10, 10])] for i in range(5)]
    rows.insert(1, [(0.85, [1, 0, 11, 10])])       # suppressed by the first: takes no slot of the three
    s, b = table(rows)
    (boxes, scores, labels), = RP.stage_b_ref(s, b, [6], 0.05, 0.01, 0.5, 3)
    assert scores.tolist() == [F32(0.9), F32(0.8), F32(0.7)] and boxes[:, 0].tolist() == [0, 20, 40]
    # two images: the offsets split the table, each image is cut on its own
    res = RP.stage_b_ref(s, b, [2, 4], 0.05, 0.01, 0.5, 3)
    assert [r[1].tolist() for r in res] == [[F32(0.9)], [F32(0.8), F32(0.7), F32(0.6)]]


def test_score_threshold_is_strict_and_min_size_is_inclusive():
    s, b = table([[(0.05, [0, 0, 10, 10])], [(0.06, [20, 0, 20.01, 10])], [(0.07, [40, 0, 40.005, 10])], [(np.nan, [60, 0, 70, 10])]])
    (boxes, scores, labels), = RP.stage_b_ref(s, b, [4], F32(0.05), F32(20.01) - F32(20), 0.5, 100)
    assert scores.tolist() == [F32(0.06)]


def test_stage_a_by_hand():
    """logits (0, ln 3): scores 1/4, 3/4.  Zero deltas give the proposal back; dw = 5 ln 2 under weight 5 doubles the width; a dw
    beyond bbox_xform_clip is cut there (exp = 62.5) and the box then clipped to the image; a proposal outside the image is clipped
    to nothing and does not survive min_size; a NaN logit voids its row."""
    ln2 = math.log(2.0)
    logits = np.array([[0, math.log(3.0)]] * 4 + [[np.nan, 0.0]], dtype=F32)
    deltas = np.zeros((5, 8), dtype=F32)
    deltas[1, 6] = 5 * ln2
    deltas[2, 6] = 100.0
    props = np.array([[10, 20, 30, 60], [10, 20, 30, 60], [10, 20, 30, 60], [200, 10, 220, 30], [10, 20, 30, 60]], dtype=F32)
    s, b = RP.stage_a_ref(logits, deltas, props, [5], [(100, 120)], WEIGHTS, CLIP)
    assert s.shape == (5, 1) and b.shape == (5, 1, 4)
    np.testing.assert_allclose(s[:4, 0], 0.75, rtol=1e-7)
    assert np.isnan(s[4, 0])
    np.testing.assert_allclose(b[0, 0], [10, 20, 30, 60], atol=1e-12)
    np.testing.assert_allclose(b[1, 0], [0, 20, 40, 60], atol=1e-5)
    # the third box: clip is taken as the f32 number the kernel receives
    half = 0.5 * math.exp(float(F32(CLIP))) * 20
    assert half > 600 and b[2, 0].tolist() == [0, 20, 120, 60]
    assert b[3, 0].tolist() == [120, 10, 120, 30]
    # rows 0, 1, 2 survive (equal scores: in row order; their IoUs are about 1/2, 1/6 and 1/3, all below 0.6); rows 3 and 4 do not
    (boxes, scores, labels), = RP.stage_b_ref(s.astype(F32), b.astype(F32), [5], 0.05, 0.01, 0.6, 100)
    assert labels.tolist() == [1, 1, 1] and boxes[0].tolist() == [10, 20, 30, 60] and boxes[2].tolist() == [0, 20, 120, 60]
    np.testing.assert_allclose(boxes[1], [0, 20, 40, 60], atol=1e-4)


# (counts, C, image sizes, D, seed): seeds for which the torch path alone satisfies the precondition below
TORCH_CASES = [((40, 0, 25), 5, ((120, 160), (90, 90), (200, 140)), 100, 1),
               ((64, 30), 7, ((150, 150), (100, 180)), 10, 2),
               ((1, 100), 2, ((80, 80), (160, 160)), 100, 6)]


@pytest.mark.parametrize('counts,C,sizes,D,seed', TORCH_CASES)
def test_reference_equals_the_torch_path_on_cpu(S, counts, C, sizes, D, seed):
    """stage A (float64) -> f32 -> stage B against `RoIHeads.postprocess_detections` on CPU tensors (the loop of torch ops): the same
    counts and labels, boxes within 1e-3 px, scores within 1e-5.  Precondition, asserted on the torch path's OWN candidate table: no
    decided IoU within 1e-3 of the NMS threshold, no score within 1e-5 of the score threshold, no two distinct adjacent scores of
    an image's ordered list within 1e-5 of each other, no box side within 1e-3 of min_size."""
    from sc2bench_amd import detection
    logits, deltas, props = RP.random_case(counts, C, sizes, seed)
    heads = detection.RoIHeads(None, None, None, score_thresh=0.05, nms_thresh=0.5, detections_per_img=D)
    tl, td = torch.from_numpy(logits), torch.from_numpy(deltas)
    tp = list(torch.from_numpy(props).split(list(counts), 0))
    with torch.no_grad():
        got = heads.postprocess_detections(tl, td, tp, list(sizes))
        t_boxes = heads.box_coder.decode(td, tp)
        t_boxes = torch.cat([detection.clip_boxes_to_image(b, hw) for b, hw in zip(t_boxes.split(list(counts), 0), sizes)])
        t_scores = torch.softmax(tl, -1)
    m = RP.margins(t_scores[:, 1:].numpy(), t_boxes[:, 1:].numpy(), counts, 0.05, 0.01, 0.5)
    assert m['iou'] > 1e-3 and m['score'] > 1e-5 and m['gap'] > 1e-5 and m['side'] > 1e-3, 'seed {}: {}; pick another seed'.format(seed, m)
    s, b = RP.stage_a_ref(logits, deltas, props, counts, sizes, heads.box_coder.weights, heads.box_coder.bbox_xform_clip)
    assert np.abs(s - t_scores[:, 1:].numpy()).max() <= 1e-6 and np.abs(b - t_boxes[:, 1:].numpy()).max() <= 1e-3
    want = RP.stage_b_ref(s.astype(F32), b.astype(F32), counts, 0.05, 0.01, 0.5, D)
    assert any(w[1].shape[0] == D for w in want) or D == 100
    for i, (wb, ws, wl) in enumerate(want):
        assert got[2][i].dtype == torch.int64 and got[2][i].tolist() == wl.tolist(), 'image {}'.format(i)
        assert got[0][i].shape == (wl.shape[0], 4)
        if wl.shape[0]:
            assert np.abs(got[0][i].numpy() - wb).max() <= 1e-3 and np.abs(got[1][i].numpy() - ws).max() <= 1e-5
    assert sum(w[2].shape[0] for w in want) > 10
