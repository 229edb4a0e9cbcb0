"""Independent references of the two detection TRAINING kernels (include/sc2_bottleneck.h: sc2_box_match, sc2_roi_align_backward),
written from the definitions and not imported from the package, plus the inputs and the stand-in detector the CPU and GPU tests share.

* `match_ref`: numpy float32, every operation rounded once and in the header's order; the maximum over the gt boxes is a SEQUENTIAL
  running maximum in ascending gt index that only a strictly greater value replaces (vectorised over the candidates, which are
  independent of each other), so that its decisions are the kernel's bit for bit.
* `roi_align_backward_ref`: float64, the adjoint of `ref_detection.roi_align_ref` built from `ref_detection.roi_samples`; it also
  returns, per map element, the number n of samples that touch it and A = sum |g| / S^2 over those samples (the test's bound).
"""
from collections import OrderedDict

import numpy as np

import ref_detection as RD

F32 = np.float32


# ------------------------------------------------------------------------------------------------ matcher
def iou_row(g, cand):
    """f32 IoU of ONE gt box g [4] with the candidates [A,4] -> f32 [A] (torchvision's box_iou, one rounding per operation)"""
    g = np.asarray(g, dtype=F32)
    c = np.ascontiguousarray(cand, dtype=F32)
    with np.errstate(invalid='ignore', divide='ignore'):
        area_g = (g[2] - g[0]) * (g[3] - g[1])
        area_c = (c[:, 2] - c[:, 0]) * (c[:, 3] - c[:, 1])
        w = np.maximum(F32(0), np.minimum(g[2], c[:, 2]) - np.maximum(g[0], c[:, 0]))
        h = np.maximum(F32(0), np.minimum(g[3], c[:, 3]) - np.maximum(g[1], c[:, 1]))
        inter = w * h
        iou = inter / (area_g + area_c - inter)
    assert iou.dtype == F32
    return iou


def match_ref(gt, cand, low, high, allow_low_quality):
    """one image: gt f32 [G,4], cand f32 [A,4] -> (matches int32 [A], best_iou f32 [A], restored bool [A], tied bool [A]).
    `tied`: the maximum (> 0) is attained by more than one gt box; `restored`: the low-quality rule applies to the candidate."""
    gt = np.asarray(gt, dtype=F32).reshape(-1, 4)
    cand = np.asarray(cand, dtype=F32).reshape(-1, 4)
    G, A = gt.shape[0], cand.shape[0]
    if G == 0:
        return np.full(A, -1, dtype=np.int32), np.zeros(A, dtype=F32), np.zeros(A, dtype=bool), np.zeros(A, dtype=bool)
    best = np.full(A, -np.inf, dtype=F32)
    idx = np.zeros(A, dtype=np.int32)
    attained = np.zeros(A, dtype=np.int64)
    rows = []
    for g in range(G):                              # the sequential walk over the gt boxes
        v = iou_row(gt[g], cand)
        rows.append(v)
        greater = v > best                          # a NaN compares false: never the maximum
        attained = np.where(greater, 1, attained + (v == best))
        best = np.where(greater, v, best)
        idx = np.where(greater, g, idx).astype(np.int32)
    restored = np.zeros(A, dtype=bool)
    for g in range(G):                              # per-gt maximum over the candidates, NaNs left out
        v = rows[g]
        top = F32(-np.inf)
        for x in v[~np.isnan(v)]:
            if x > top:
                top = x
        restored |= (v == top)
    low, high = F32(low), F32(high)
    matches = np.where(best < low, -1, np.where(best < high, -2, idx)).astype(np.int32)
    if allow_low_quality:
        matches = np.where(restored, idx, matches).astype(np.int32)
    return matches, best, restored, (attained > 1) & (best > 0)


def match_ref_batch(gts, cands, low, high, allow_low_quality):
    """several images -> (matches int32 [sum A], best_iou f32 [sum A])"""
    out = [match_ref(g, c, low, high, allow_low_quality) for g, c in zip(gts, cands)]
    return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])


def match_boxes_case(A, G, seed):
    """clustered random boxes: G gt boxes and A candidates over the same extent"""
    gt = RD.random_boxes(G, 1, seed=1000 + seed)[0] if G else np.zeros((0, 4), dtype=F32)
    cand = RD.random_boxes(A, 1, seed=seed)[0]
    return gt, cand


# ------------------------------------------------------------------------------------------------ RoIAlign backward
TOUCH = 1.0 + RD.EXCLUDE      # a sample "touches" the pixels within this distance per axis: the closed bilinear support, widened by
#                               the band within which an f32 sample may fall on the other side of a pixel boundary


def _axis(samples, size):
    """float64 per-axis weights of torchvision's bilinear_interpolate: -> (W [n, size], T bool [n, size]); an invalid sample
    (outside [-1, size]) has an all-zero row in both"""
    n = len(samples)
    Wt, T = np.zeros((n, size)), np.zeros((n, size), dtype=bool)
    for i, y in enumerate(samples):
        if y < -1.0 or y > size:
            continue
        y = max(y, 0.0)
        lo = int(y)
        if lo >= size - 1:
            hi = lo = size - 1
            y = float(lo)
        else:
            hi = lo + 1
        l = y - lo
        Wt[i, lo] += 1.0 - l
        Wt[i, hi] += l
        T[i] = np.abs(np.arange(size) - y) < TOUCH
    return Wt, T


def roi_align_backward_ref(grad_out, map_sizes, scales, rois, levels, n_images, P, S):
    """grad_out [K,C,P,P], rois [K,5], levels [K] -> (grads, n, A): lists per level of float64 [N,C,H,W], int64 [N,H,W],
    float64 [N,C,H,W].  A RoI whose level or image does not exist contributes nothing."""
    g = np.asarray(grad_out, dtype=np.float64)
    K, C = g.shape[0], g.shape[1]
    grads = [np.zeros((n_images, C, h, w)) for h, w in map_sizes]
    cnt = [np.zeros((n_images, h, w), dtype=np.int64) for h, w in map_sizes]
    mag = [np.zeros((n_images, C, h, w)) for h, w in map_sizes]
    for k in range(K):
        lvl, img = int(levels[k]), float(rois[k][0])
        if not (0 <= lvl < len(map_sizes)) or not (0 <= img < n_images):
            continue
        img = int(img)
        h, w = map_sizes[lvl]
        ys, xs = RD.roi_samples(np.asarray(rois[k][1:], dtype=np.float64), float(scales[lvl]), P, S)
        Wy, Ty = _axis(ys, h)
        Wx, Tx = _axis(xs, w)
        gs = np.repeat(np.repeat(g[k], S, axis=1), S, axis=2) / float(S * S)          # [C, PS, PS]: per sample
        rs, cs = np.nonzero(Ty.any(0))[0], np.nonzero(Tx.any(0))[0]
        if rs.size == 0 or cs.size == 0:
            continue
        r0, r1, c0, c1 = rs[0], rs[-1] + 1, cs[0], cs[-1] + 1
        Wy_, Wx_, Ty_, Tx_ = Wy[:, r0:r1], Wx[:, c0:c1], Ty[:, r0:r1].astype(np.float64), Tx[:, c0:c1].astype(np.float64)
        grads[lvl][img, :, r0:r1, c0:c1] += np.einsum('iy,cij,jx->cyx', Wy_, gs, Wx_)
        mag[lvl][img, :, r0:r1, c0:c1] += np.einsum('iy,cij,jx->cyx', Ty_, np.abs(gs), Tx_)
        cnt[lvl][img, r0:r1, c0:c1] += np.rint(np.outer(Ty_.sum(0), Tx_.sum(0))).astype(np.int64)
    return grads, cnt, mag


def roi_backward_bound(cnt, mag):
    """|err| <= (2^-13 + n * 2^-24) * A per element"""
    return [(2.0 ** -13 + c[:, None].astype(np.float64) * 2.0 ** -24) * m for c, m in zip(cnt, mag)]


# ------------------------------------------------------------------------------------------------ the stand-in detector
STANDIN_IMAGE = (64, 96)
STANDIN_CLASSES = 5


def standin_targets(device='cpu'):
    """two images: two gt boxes (one of them exactly an anchor of the coarse level), and none"""
    import torch
    return [{'boxes': torch.tensor([[8.0, 8.0, 40.0, 40.0], [50.0, 20.0, 90.0, 60.0]], device=device),
             'labels': torch.tensor([1, 3], dtype=torch.int64, device=device)},
            {'boxes': torch.zeros((0, 4), device=device), 'labels': torch.zeros((0,), dtype=torch.int64, device=device)}]


def standin_images(device='cpu', seed=3):
    import torch
    g = torch.Generator().manual_seed(seed)
    H, W = STANDIN_IMAGE
    return [torch.rand(3, H, W, generator=g).to(device), torch.rand(3, H, W, generator=g).to(device)]


def standin_model(detection, seed=5):
    """a FasterRCNN with its training path switched on, over a two-level, 8-channel stand-in backbone (strides 4 and 8) for 64 x 96 images"""
    import torch
    from torch import nn

    class TwoLevel(nn.Module):
        out_channels = 8

        def __init__(self):
            super().__init__()
            self.conv1 = nn.Conv2d(3, 8, 3, stride=4, padding=1)
            self.conv2 = nn.Conv2d(8, 8, 3, stride=2, padding=1)

        def forward(self, x):
            a = torch.relu(self.conv1(x))
            return OrderedDict([('0', a), ('1', torch.relu(self.conv2(a)))])

    torch.manual_seed(seed)
    H, W = STANDIN_IMAGE
    return detection.enable_training(detection.FasterRCNN(
        TwoLevel(), min_size=H, max_size=W, rpn_anchor_generator=detection.AnchorGenerator(((16,), (32,)), ((0.5, 1.0, 2.0),) * 2),
        box_roi_pool=detection.MultiScaleRoIAlign(['0', '1'], 7, 2), box_head=detection.TwoMLPHead(8 * 49, 32),
        box_predictor=detection.FastRCNNPredictor(32, STANDIN_CLASSES), rpn_batch_size_per_image=64, box_batch_size_per_image=64,
        rpn_pre_nms_top_n_train=200, rpn_post_nms_top_n_train=100, rpn_post_nms_top_n_test=50, box_score_thresh=0.0))
