"""tests/ref_rpn_post.py (the restatement the GPU tests of sc2_rpn_proposals compare against) pinned without a GPU: on hand-worked
cases, and against the package's own torch-op `RegionProposalNetwork.filter_proposals` on the CPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_rpn_post as RR  # noqa: E402

F32 = np.float32
WEIGHTS = (1.0, 1.0, 1.0, 1.0)
CLIP = math.log(1000.0 / 16)


def table(levels, K=None):
    """levels: per level a list of (score, box) by rank -> (scores f32 [1,L,K], boxes f32 [1,L,K,4], k [1,L]) of one image"""
    K = K or max(len(l) for l in levels)
    s, b, k = np.zeros((1, len(levels), K), dtype=F32), np.zeros((1, len(levels), K, 4), dtype=F32), np.zeros((1, len(levels)), dtype=np.int32)
    for l, rows in enumerate(levels):
        k[0, l] = len(rows)
        for j, (score, box) in enumerate(rows):
            s[0, l, j], b[0, l, j] = score, box
    return s, b, k


def test_equal_logits_across_the_cut_go_by_the_lower_index():
    assert RR.select_ref(np.array([1, 5, 5, 5, 0], dtype=F32), 2).tolist() == [1, 2]
    assert RR.select_ref(np.array([5, 1, 5, 7, 5], dtype=F32), 3).tolist() == [3, 0, 2]
    assert RR.select_ref(np.full(9, 0.25, dtype=F32), 4).tolist() == [0, 1, 2, 3]


def test_nan_is_selected_first_and_dropped_at_the_score_test():
    logits = np.array([0.0, np.nan, 3.0, np.nan, -np.inf, np.inf], dtype=F32)
    assert RR.select_ref(logits, 4).tolist() == [1, 3, 5, 2]
    assert RR.select_ref(logits, 6).tolist() == [1, 3, 5, 2, 0, 4]
    box = [0, 0, 10, 10]
    s, b, k = table([[(np.nan, box), (0.9, [20, 0, 30, 10])]])
    (boxes, scores, levels, ranks), = RR.stage_b_ref(s, b, k, 0.0, 1e-3, 0.7, 100)
    assert scores.tolist() == [F32(0.9)] and ranks.tolist() == [1]
    # ... with a negative threshold too: a comparison with a NaN is false
    assert RR.stage_b_ref(s, b, k, -1.0, 1e-3, 0.7, 100)[0][3].tolist() == [1]


def test_zeros_of_either_sign_tie():
    assert RR.select_ref(np.array([-0.0, 0.0, -0.0, 1.0, -1.0], dtype=F32), 4).tolist() == [3, 0, 1, 2]
    assert RR.select_ref(np.array([0.0, -0.0], dtype=F32), 1).tolist() == [0] and RR.select_ref(np.array([-0.0, 0.0], dtype=F32), 1).tolist() == [0]


def test_a_level_smaller_than_k():
    assert RR.select_ref(np.array([1.0, 2.0], dtype=F32), 5).tolist() == [1, 0]
    obj = [np.array([[[[1.0, 2.0]]]], dtype=F32), np.arange(12, dtype=F32).reshape(1, 3, 2, 2)]
    index, k = RR.select_batch(obj, 5)
    assert k.tolist() == [[2, 5]] and index[0, 0].tolist() == [1, 0, -1, -1, -1]
    # level 1: the map [A=3, H=2, W=2] holds 0..11 in memory order a (h w): index t = (h W + w) A + a, so value 11 sits at t = 3 * 3 + 2
    assert RR.level_logits(obj[1])[0].tolist() == [0, 4, 8, 1, 5, 9, 2, 6, 10, 3, 7, 11]
    assert index[0, 1].tolist() == [11, 8, 5, 2, 10]


def test_score_threshold_and_min_size_are_inclusive():
    side = F32(20.5) - F32(20)
    s, b, k = table([[(0.5, [0, 0, 10, 10]), (0.49999997, [20, 0, 30, 10]), (0.75, [40, 0, 40.5, 10]), (0.8, [60, 0, 60.25, 10])]])
    (boxes, scores, levels, ranks), = RR.stage_b_ref(s, b, k, 0.5, side, 0.7, 100)
    assert ranks.tolist() == [2, 0]           # score == threshold stays, side == min_size stays; below either goes


def test_two_levels_never_suppress_each_other():
    box = [0, 0, 10, 10]
    s, b, k = table([[(0.9, box), (0.8, box)], [(0.9, box), (0.7, [100, 0, 110, 10])]])
    (boxes, scores, levels, ranks), = RR.stage_b_ref(s, b, k, 0.0, 1e-3, 0.7, 100)
    assert levels.tolist() == [0, 1, 1] and ranks.tolist() == [0, 0, 1] and scores.tolist() == [F32(0.9), F32(0.9), F32(0.7)]


def test_saturated_scores_the_lower_level_goes_first():
    """logits 17 and 20 both give 1.0f; the key order is (score descending, level ascending, rank ascending)"""
    with np.errstate(all='ignore'):
        assert [float(F32(1) / (F32(1) + np.exp(F32(-x)))) for x in (17.0, 20.0)] == [1.0, 1.0]
    far = lambda i: [100.0 * i, 0, 100.0 * i + 10, 10]      # noqa: E731
    s, b, k = table([[(1.0, far(0)), (0.5, far(1)), (0.25, far(2))], [(1.0, far(3)), (1.0, far(4)), (0.5, far(5))]])
    (boxes, scores, levels, ranks), = RR.stage_b_ref(s, b, k, 0.0, 1e-3, 0.7, 4)
    assert levels.tolist() == [0, 1, 1, 0] and ranks.tolist() == [0, 0, 1, 1] and boxes[:, 0].tolist() == [0, 300, 400, 100]


def test_the_cut_at_p_comes_after_the_suppression():
    rows = [(0.9 - 0.1 * i, [20.0 * i, 0, 20.0 * i + 10, 10]) for i in range(5)]
    rows.insert(1, (0.85, [1, 0, 11, 10]))       # IoU 9 / 11 with the first: suppressed, takes no slot of the three
    s, b, k = table([rows])
    (boxes, scores, levels, ranks), = RR.stage_b_ref(s, b, k, 0.0, 1e-3, 0.7, 3)
    assert ranks.tolist() == [0, 2, 3] and boxes[:, 0].tolist() == [0, 20, 40]
    # slots behind k are not candidates, whatever they hold
    s[0, 0, 5], k[0, 0] = 0.99, 5
    assert RR.stage_b_ref(s, b, k, 0.0, 1e-3, 0.7, 100)[0][3].tolist() == [0, 2, 3, 4]


def test_stage_a_by_hand():
    """logit ln 3: score 3/4.  Zero deltas give the anchor back; dw = ln 2 doubles the width; a dw beyond bbox_xform_clip is cut
    there (exp = 62.5) and the box then clipped to the image; an anchor outside the image is clipped to nothing."""
    obj = [np.full((1, 1, 1, 4), math.log(3.0), dtype=F32)]
    dl = [np.zeros((1, 4, 1, 4), dtype=F32)]
    dl[0][0, 2, 0, 1] = math.log(2.0)
    dl[0][0, 2, 0, 2] = 100.0
    anchors = np.array([[10, 20, 30, 60], [10, 20, 30, 60], [10, 20, 30, 60], [200, 10, 220, 30]], dtype=F32)
    index, k = np.array([[[0, 1, 2, 3, -1]]], dtype=np.int32), np.array([[4]], dtype=np.int32)
    s, b = RR.stage_a_ref(obj, dl, anchors, [(100, 120)], index, k, WEIGHTS, CLIP)
    assert s.shape == (1, 1, 5) and b.shape == (1, 1, 5, 4) and s[0, 0, 4] == 0 and not b[0, 0, 4].any()
    np.testing.assert_allclose(s[0, 0, :4], 0.75, rtol=1e-7)
    np.testing.assert_allclose(b[0, 0, 0], [10, 20, 30, 60], atol=1e-12)
    np.testing.assert_allclose(b[0, 0, 1], [0, 20, 40, 60], atol=1e-5)
    assert b[0, 0, 2].tolist() == [0, 20, 120, 60] and b[0, 0, 3].tolist() == [120, 10, 120, 30]
    (boxes, scores, levels, ranks), = RR.stage_b_ref(s.astype(F32), b.astype(F32), k, 0.0, 1e-3, 0.7, 100)
    assert ranks.tolist() == [0, 1, 2]         # equal scores: by rank; the IoUs are 1/2, 1/6 and 1/3; the empty box is dropped


# (level shapes, image sizes, K, P, seed): seeds for which the torch path alone satisfies the precondition below
TORCH_CASES = [([(3, 4, 5), (3, 2, 3), (3, 1, 2)], ((120, 160), (100, 150)), 40, 1000, 1),
               ([(1, 6, 8), (3, 3, 4)], ((96, 128), (96, 100), (80, 128)), 30, 20, 0),
               ([(3, 5, 6)], ((100, 120),), 1000, 1000, 0)]


@pytest.mark.parametrize('shapes,sizes,K,P,seed', TORCH_CASES)
def test_reference_equals_the_torch_path_on_cpu(S, shapes, sizes, K, P, seed):
    """select -> stage A (float64) -> f32 -> stage B against `RegionProposalNetwork.filter_proposals` on CPU tensors (concat, decode
    of every anchor, topk per level, the per-image loop): the same kept sets in the same order, boxes within 1e-3 px, scores within
    1e-5.  The logits of an image are a permutation of distinct values (torch.topk leaves ties unspecified).  Precondition, asserted
    on the torch path's OWN table: no decided IoU within 1e-3 of the NMS threshold, no score within 1e-5 of the score threshold, no
    two distinct adjacent scores of an image's ordered list within 1e-5 of each other, no box side within 1e-3 of min_size."""
    from sc2bench_amd import detection
    obj, dl, anchors = RR.random_case(shapes, len(sizes), max(sizes), seed, logit_scale=3.0, distinct=True)
    rpn = detection.RegionProposalNetwork(None, None, pre_nms_top_n=dict(training=K, testing=K), post_nms_top_n=dict(training=P, testing=P),
                                          score_thresh=0.3).eval()
    rpn.min_size = 0.5        # (a box clipped to nothing has side 0: half a pixel away from the test on either path)
    N = len(sizes)
    with torch.no_grad():
        flat_obj, flat_dl = detection.concat_box_prediction_layers([torch.from_numpy(o) for o in obj], [torch.from_numpy(d) for d in dl])
        t_anchors = [torch.from_numpy(anchors)] * N
        proposals = rpn.box_coder.decode(flat_dl, t_anchors).view(N, -1, 4)
        got_boxes, got_scores = rpn.filter_proposals(proposals, flat_obj, list(sizes), [a * h * w for a, h, w in shapes])
        t_boxes = torch.stack([detection.clip_boxes_to_image(p, hw) for p, hw in zip(proposals, sizes)]).numpy()
        t_scores = torch.sigmoid(flat_obj).view(N, -1).numpy()
    index, k = RR.select_batch(obj, K)
    # the torch path's table of the reference's selection
    sel_s, sel_b, off = np.zeros(index.shape, dtype=F32), np.zeros(index.shape + (4,), dtype=F32), 0
    for l, (a, h, w) in enumerate(shapes):
        for i in range(N):
            t = index[i, l, :k[i, l]]
            sel_s[i, l, :k[i, l]], sel_b[i, l, :k[i, l]] = t_scores[i, off + t], t_boxes[i, off + t]
        off += a * h * w
    m = RR.margins(sel_s, sel_b, k, rpn.score_thresh, rpn.min_size, rpn.nms_thresh)
    assert m['iou'] > 1e-3 and m['score'] > 1e-5 and m['gap'] > 1e-5 and m['side'] > 1e-3, 'seed {}: {}; pick another seed'.format(seed, m)
    s, b = RR.stage_a_ref(obj, dl, anchors, sizes, index, k, rpn.box_coder.weights, rpn.box_coder.bbox_xform_clip)
    assert np.abs(s - sel_s).max() <= 1e-6 and np.abs(b - sel_b).max() <= 1e-3
    want = RR.stage_b_ref(s.astype(F32), b.astype(F32), k, rpn.score_thresh, rpn.min_size, rpn.nms_thresh, P)
    assert any(w[1].shape[0] == P for w in want) or P == 1000
    for i, (wb, ws, wl, wr) in enumerate(want):
        assert got_boxes[i].shape == (ws.shape[0], 4) and got_scores[i].shape == (ws.shape[0],), 'image {}'.format(i)
        if ws.shape[0]:
            assert np.abs(got_boxes[i].numpy() - wb).max() <= 1e-3 and np.abs(got_scores[i].numpy() - ws).max() <= 1e-5
            # the same candidates, not merely close ones: each kept box is the torch path's box of that (level, rank)
            assert np.abs(sel_b[i][wl, wr] - got_boxes[i].numpy()).max() == 0
    assert sum(w[1].shape[0] for w in want) > 10
