"""The detection tail of Faster R-CNN behind the feature pyramid: a torch-only restatement of the INFERENCE path of
torchvision's `FasterRCNN` (anchor generator, RPN, multi-scale RoIAlign, box head, RoI heads, image transform), under
torchvision's module and parameter names so that its checkpoints load (sc2bench/models/detection/rcnn.py builds the
reference's detector from these classes).

No torchvision binary exists here to pin this file against: every semantic below is **[recalled: torchvision 0.15+]** in
the sense of SURVEY.md section 8(c) -- written down from the published source as remembered, not compared against a run.

Two operations have no torch operator and run on the library's kernels (csrc/detect.hip) for device tensors:
non-maximum suppression (`nms`, `batched_nms` -> `hip.batched_nms`) and RoIAlign (`roi_align`, `multiscale_roi_align` ->
`hip.roi_align`).  CPU tensors, and device tensors while `hip.host_policy.nms_hip` / `roi_align_hip` are off (A/B), take a
torch-op implementation of the same definitions (include/sc2_bottleneck.h states them; tests/ref_detection.py restates
them independently).  The RoI heads' `postprocess_detections` runs for the whole batch on csrc/det_post.hip (`hip.det_postprocess`:
softmax, decode, clip, the two filters, per-class NMS and the first `detections_per_img`, three launches and one read-back) for f32
device tensors while `hip.host_policy.det_post_hip` is on; otherwise, and for a batch above that kernel's candidate caps, the
per-image loop of torch ops around `batched_nms` (tests/ref_det_post.py restates the stage).  The RPN's proposal selection runs
the same way on csrc/rpn_post.hip (`hip.rpn_proposals`: the top-k of each level with ties by the lower index, sigmoid, decode and
clip of the selected anchors, per-level NMS and the first `post_nms_top_n`, three launches on the head's maps as they stand and
one read-back) for f32 device maps while `hip.host_policy.rpn_post_hip` is on; otherwise, and outside that kernel's caps, concat,
full decode and `filter_proposals` (tests/ref_rpn_post.py restates the stage).  Everything else is small tensor algebra and two
small GEMM stacks on torch ops.

`RCNNTransformWithCompression` (sc2bench/models/detection/transform.py) is the transform of the input-compression baseline: a
codec between resize and normalise; for plain JPEG on device images it runs on csrc/rcnn_input.hip + csrc/jpeg_image.hip.

TRAINING (torchvision's loss path, **[recalled: torchvision 0.15+]** like the rest) is an opt-in: behind `enable_training(model)`
(which `training.DistillationStage` calls for a `forward_proc: 'forward_batch_target'` student) `FasterRCNN.forward(images,
targets)` in training mode returns the four-key loss dict (`loss_classifier`, `loss_box_reg`, `loss_objectness`, `loss_rpn_box_reg`).  Two pieces of
it run on the library's kernels for device tensors: the proposal matcher (`match_boxes` -> `hip.box_match`: `Matcher` over `box_iou`
for all images of the batch in one call, without the [G, A] IoU matrix) and the backward of multi-level RoIAlign (`_RoIAlignFn` ->
`hip.roi_align` / `hip.roi_align_backward`, f32 maps only: the bf16 forward stays inference-only).  CPU tensors, and device tensors
while `hip.host_policy.box_match_hip` / `roi_align_bwd_hip` are off (A/B), take the torch-op definitions (`box_iou` + `Matcher`;
autograd through `_roi_align_level_torch`); both routes give the same matches.  Box encoding, the balanced sampler, smooth-L1, BCE
and CE are small tensor algebra on at most a few thousand sampled rows and stay on torch ops.  Not built: the COCO dataset side
(transforms, aspect-ratio grouping), mask and keypoint heads, a bf16 backward, the random choice among several `min_size` values.
"""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F
from torch import nn

from . import hip
from .analysis import AnalyzableModule
from .transforms import AdaptivePad, Compose, DeferredDetBatch, PILImageModule, to_pil_image, to_tensor

BBOX_XFORM_CLIP = math.log(1000.0 / 16)


# ------------------------------------------------------------------------------------------------ box algebra
def clip_boxes_to_image(boxes, size):
    height, width = size
    x = boxes[..., 0::2].clamp(min=0, max=width)
    y = boxes[..., 1::2].clamp(min=0, max=height)
    return torch.stack((x, y), dim=boxes.dim()).reshape(boxes.shape)


def remove_small_boxes(boxes, min_size):
    ws, hs = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
    return torch.where((ws >= min_size) & (hs >= min_size))[0]


class BoxCoder(object):
    """Box regression deltas <-> boxes (torchvision.models.detection._utils.BoxCoder): `decode` at inference, `encode` for the regression targets in training."""

    def __init__(self, weights, bbox_xform_clip=BBOX_XFORM_CLIP):
        self.weights = weights
        self.bbox_xform_clip = bbox_xform_clip

    def encode(self, reference_boxes, proposals):
        """lists of [k_i,4] per image (the matched gt boxes, the anchors / proposals) -> the list of regression targets [k_i,4]"""
        boxes_per_image = [len(b) for b in reference_boxes]
        targets = self.encode_single(torch.cat(list(reference_boxes), dim=0), torch.cat(list(proposals), dim=0))
        return targets.split(boxes_per_image, 0)

    def encode_single(self, reference_boxes, proposals):
        """torchvision's `encode_boxes`: dx = wx * (gt_ctr_x - ctr_x) / width, dw = ww * log(gt_width / width); dy, dh likewise"""
        wx, wy, ww, wh = torch.as_tensor(self.weights, dtype=reference_boxes.dtype, device=reference_boxes.device).unbind(0)
        px1, py1, px2, py2 = [c.unsqueeze(1) for c in proposals.to(reference_boxes.dtype).unbind(1)]
        gx1, gy1, gx2, gy2 = [c.unsqueeze(1) for c in reference_boxes.unbind(1)]
        ex_w, ex_h = px2 - px1, py2 - py1
        ex_cx, ex_cy = px1 + 0.5 * ex_w, py1 + 0.5 * ex_h
        gt_w, gt_h = gx2 - gx1, gy2 - gy1
        gt_cx, gt_cy = gx1 + 0.5 * gt_w, gy1 + 0.5 * gt_h
        return torch.cat((wx * (gt_cx - ex_cx) / ex_w, wy * (gt_cy - ex_cy) / ex_h, ww * torch.log(gt_w / ex_w), wh * torch.log(gt_h / ex_h)), dim=1)

    def decode(self, rel_codes, boxes):
        concat = torch.cat(list(boxes), dim=0)
        box_sum = concat.shape[0]
        pred = self.decode_single(rel_codes, concat)
        if box_sum > 0:
            pred = pred.reshape(box_sum, -1, 4)
        return pred

    def decode_single(self, rel_codes, boxes):
        boxes = boxes.to(rel_codes.dtype)
        widths, heights = boxes[:, 2] - boxes[:, 0], boxes[:, 3] - boxes[:, 1]
        ctr_x, ctr_y = boxes[:, 0] + 0.5 * widths, boxes[:, 1] + 0.5 * heights
        wx, wy, ww, wh = self.weights
        dx, dy = rel_codes[:, 0::4] / wx, rel_codes[:, 1::4] / wy
        dw = torch.clamp(rel_codes[:, 2::4] / ww, max=self.bbox_xform_clip)
        dh = torch.clamp(rel_codes[:, 3::4] / wh, max=self.bbox_xform_clip)
        pred_ctr_x, pred_ctr_y = dx * widths[:, None] + ctr_x[:, None], dy * heights[:, None] + ctr_y[:, None]
        half_w, half_h = 0.5 * (torch.exp(dw) * widths[:, None]), 0.5 * (torch.exp(dh) * heights[:, None])
        return torch.stack((pred_ctr_x - half_w, pred_ctr_y - half_h, pred_ctr_x + half_w, pred_ctr_y + half_h), dim=2).flatten(1)


# ------------------------------------------------------------------------------------------------ matcher, sampler, loss
def box_iou(boxes1, boxes2):
    """torchvision.ops.box_iou: [G,4], [A,4] -> [G,A]; every operation its own op (rounded once, as sc2_box_match does):
    areas (x2 - x1) * (y2 - y1), wh = (min(rb) - max(lt)).clamp(0), inter / (area1 + area2 - inter)"""
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    wh = (torch.min(boxes1[:, None, 2:], boxes2[:, 2:]) - torch.max(boxes1[:, None, :2], boxes2[:, :2])).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


class Matcher(object):
    """torchvision.models.detection._utils.Matcher over a [G, A] quality matrix -> int64 [A]: the gt index, BELOW_LOW_THRESHOLD where
    the maximum is < low, BETWEEN_THRESHOLDS where it is >= low and < high.  `allow_low_quality_matches`: every candidate whose
    quality with some gt box equals that box's maximum over all candidates gets its own argmax back (torchvision's known behaviour:
    the argmax, not the gt box it is best for).  Stated where torchvision leaves it open, as include/sc2_bottleneck.h does for
    sc2_box_match: a tie goes to the lowest gt index, and a NaN quality (0 / 0) is never a maximum (a column of NaNs: index 0, below
    the threshold)."""
    BELOW_LOW_THRESHOLD = -1
    BETWEEN_THRESHOLDS = -2

    def __init__(self, high_threshold, low_threshold, allow_low_quality_matches=False):
        if low_threshold > high_threshold:
            raise ValueError('Matcher: low_threshold should be <= high_threshold')
        self.high_threshold, self.low_threshold = high_threshold, low_threshold
        self.allow_low_quality_matches = allow_low_quality_matches

    def __call__(self, match_quality_matrix):
        if match_quality_matrix.numel() == 0:
            if match_quality_matrix.shape[0] == 0:
                raise ValueError('No ground-truth boxes available for one of the images during training')
            raise ValueError('No proposal boxes available for one of the images during training')
        ranked = torch.where(torch.isnan(match_quality_matrix), torch.full_like(match_quality_matrix, float('-inf')), match_quality_matrix)
        matched_vals, matches = ranked.max(dim=0)
        all_matches = matches.clone() if self.allow_low_quality_matches else None
        below = matched_vals < self.low_threshold
        between = (matched_vals >= self.low_threshold) & (matched_vals < self.high_threshold)
        matches[below] = self.BELOW_LOW_THRESHOLD
        matches[between] = self.BETWEEN_THRESHOLDS
        if self.allow_low_quality_matches:
            self.set_low_quality_matches_(matches, all_matches, match_quality_matrix)
        return matches

    def set_low_quality_matches_(self, matches, all_matches, match_quality_matrix):
        ranked = torch.where(torch.isnan(match_quality_matrix), torch.full_like(match_quality_matrix, float('-inf')), match_quality_matrix)
        highest_quality_foreach_gt = ranked.max(dim=1)[0]
        restore = (match_quality_matrix == highest_quality_foreach_gt[:, None]).any(dim=0)      # (a NaN equals nothing)
        matches[restore] = all_matches[restore]


def match_boxes(gt_boxes, boxes, high_threshold, low_threshold, allow_low_quality_matches):
    """`Matcher(box_iou(gt_boxes[i], boxes[i]))` for every image i -> a list of int64 [A_i]; an image without gt boxes is all
    BELOW_LOW_THRESHOLD.  Device tensors: ONE call of `hip.box_match` for the batch (no IoU matrix); CPU tensors, or
    `hip.host_policy.box_match_hip` off: the matrix + `Matcher` per image.  Both give the same indices."""
    gt_boxes = [g.detach().to(torch.float32).reshape(-1, 4) for g in gt_boxes]
    boxes = [b.detach().to(torch.float32) for b in boxes]
    if boxes[0].is_cuda and hip.host_policy.box_match_hip:
        counts = [int(b.shape[0]) for b in boxes]
        matches, _ = hip.box_match(torch.cat(gt_boxes).contiguous(), [int(g.shape[0]) for g in gt_boxes], torch.cat(boxes).contiguous(), counts,
                                   low_threshold, high_threshold, allow_low_quality_matches, want_iou=False)
        return list(matches.to(torch.int64).split(counts))
    matcher = Matcher(high_threshold, low_threshold, allow_low_quality_matches)
    out = []
    for g, b in zip(gt_boxes, boxes):
        if g.shape[0] == 0 or b.shape[0] == 0:
            out.append(torch.full((b.shape[0],), Matcher.BELOW_LOW_THRESHOLD, dtype=torch.int64, device=b.device))
        else:
            out.append(matcher(box_iou(g, b)))
    return out


class BalancedPositiveNegativeSampler(object):
    """torchvision's sampler: per image up to batch_size_per_image * positive_fraction of the positives (label >= 1) and the rest of
    the batch from the negatives (label == 0), by two `randperm` draws per image on the labels' device from the global generator --
    positives first, then negatives -> (list of uint8 positive masks, list of uint8 negative masks)."""

    def __init__(self, batch_size_per_image, positive_fraction):
        self.batch_size_per_image, self.positive_fraction = batch_size_per_image, positive_fraction

    def __call__(self, matched_idxs):
        pos_idx, neg_idx = [], []
        for m in matched_idxs:
            positive, negative = torch.where(m >= 1)[0], torch.where(m == 0)[0]
            num_pos = min(positive.numel(), int(self.batch_size_per_image * self.positive_fraction))
            num_neg = min(negative.numel(), self.batch_size_per_image - num_pos)
            perm1 = torch.randperm(positive.numel(), device=positive.device)[:num_pos]
            perm2 = torch.randperm(negative.numel(), device=negative.device)[:num_neg]
            pos_mask, neg_mask = torch.zeros_like(m, dtype=torch.uint8), torch.zeros_like(m, dtype=torch.uint8)
            pos_mask[positive[perm1]] = 1
            neg_mask[negative[perm2]] = 1
            pos_idx.append(pos_mask)
            neg_idx.append(neg_mask)
        return pos_idx, neg_idx


def smooth_l1_loss(input, target, beta=1.0 / 9, size_average=False):
    """0.5 * d^2 / beta where |d| < beta, |d| - 0.5 * beta elsewhere, summed (or averaged)"""
    n = torch.abs(input - target)
    loss = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    return loss.mean() if size_average else loss.sum()


# ------------------------------------------------------------------------------------------------ NMS
def _nms_sorted_torch(b, g, iou_threshold, rows=1024):
    """The definition of sc2_nms on torch ops: b f32 [n,4] in processing order, g [n] -> bool keep mask [n] on b's device.
    The pair tests are evaluated `rows` rows at a time in f32 (every operation its own op: rounded once, as the kernel does),
    the greedy walk runs on the host over each chunk's bits."""
    import numpy as np
    n = b.shape[0]
    x1, y1, x2, y2 = b.unbind(1)
    area = (x2 - x1) * (y2 - y1)
    thr = torch.tensor(float(iou_threshold), dtype=torch.float32, device=b.device)
    removed, keep = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for r0 in range(0, n, rows):
        r1 = min(n, r0 + rows)
        w = (torch.min(x2[r0:r1, None], x2[None, r0:]) - torch.max(x1[r0:r1, None], x1[None, r0:])).clamp(min=0)
        h = (torch.min(y2[r0:r1, None], y2[None, r0:]) - torch.max(y1[r0:r1, None], y1[None, r0:])).clamp(min=0)
        inter = w * h
        iou = inter / (area[r0:r1, None] + area[None, r0:] - inter)
        m = ((iou > thr) & (g[r0:r1, None] == g[None, r0:])).cpu().numpy()
        for i in range(r0, r1):
            if not removed[i]:
                keep[i] = True
                removed[i + 1:] |= m[i - r0, i + 1 - r0:]
    return torch.from_numpy(keep).to(b.device)


def batched_nms(boxes, scores, idxs, iou_threshold):
    """Greedy NMS within each value of `idxs` -> int64 indices of the kept boxes by descending score (ties: lower index first).
    torchvision's "vanilla" batched NMS, not its coordinate-offset trick (see `hip.batched_nms`)."""
    if boxes.is_cuda and hip.host_policy.nms_hip:
        return hip.batched_nms(boxes, scores, idxs, iou_threshold)
    if boxes.shape[0] == 0:
        return torch.empty(0, dtype=torch.int64, device=boxes.device)
    order = torch.sort(scores, descending=True, stable=True)[1]
    b, g = boxes.detach().to(torch.float32)[order], idxs[order]
    if b.shape[0] <= 1024:
        return order[_nms_sorted_torch(b, g, iou_threshold)]
    keep = torch.zeros(b.shape[0], dtype=torch.bool, device=b.device)
    for v in torch.unique(g).tolist():        # groups are independent: far fewer pair tests group by group
        sel = torch.where(g == v)[0]
        keep[sel] = _nms_sorted_torch(b[sel], g[sel], iou_threshold)
    return order[keep]


def nms(boxes, scores, iou_threshold):
    return batched_nms(boxes, scores, torch.zeros(boxes.shape[0], dtype=torch.int32, device=boxes.device), iou_threshold)


# ------------------------------------------------------------------------------------------------ RoIAlign
def _roi_axis(c, size):
    """one axis of the bilinear sample positions c (f32): -> (valid, low, high, l, h)"""
    valid = ~((c < -1.0) | (c > float(size)))
    c = c.clamp(min=0.0)
    low = c.to(torch.int64).clamp(min=0, max=size - 1)
    edge = low >= size - 1
    high = torch.where(edge, low, low + 1)
    c = torch.where(edge, low.to(c.dtype), c)
    l = c - low.to(c.dtype)
    return valid, low, high, l, 1.0 - l


def _roi_align_level_torch(feat, rois, scale, P, S, chunk=128):
    """feat [N,C,H,W], rois f32 [k,5] -> f32 [k,C,P,P], aligned=False"""
    feat = feat.to(torch.float32)
    H, W = feat.shape[-2:]
    p = torch.arange(P, dtype=torch.float32, device=feat.device)[None, :, None]
    i = torch.arange(S, dtype=torch.float32, device=feat.device)[None, None, :]
    outs = []
    for k0 in range(0, rois.shape[0], chunk):
        r = rois[k0:k0 + chunk].to(torch.float32)
        k = r.shape[0]
        img = r[:, 0].to(torch.int64)[:, None, None]
        coords = []
        for lo, hi in ((r[:, 2], r[:, 4]), (r[:, 1], r[:, 3])):     # y, then x
            start, end = lo * scale, hi * scale
            bin_ = ((end - start).clamp(min=1.0) / P)[:, None, None]
            coords.append((start[:, None, None] + p * bin_ + (i + 0.5) * bin_ / S).reshape(k, P * S))
        vy, yl, yh, ly, hy = _roi_axis(coords[0], H)
        vx, xl, xh, lx, hx = _roi_axis(coords[1], W)

        def at(yy, xx):      # [k, PS, PS, C]
            return feat[img, :, yy[:, :, None], xx[:, None, :]]

        def wt(a, b):
            return (a[:, :, None] * b[:, None, :])[..., None]
        val = wt(hy, hx) * at(yl, xl) + wt(hy, lx) * at(yl, xh) + wt(ly, hx) * at(yh, xl) + wt(ly, lx) * at(yh, xh)
        val = val * (vy[:, :, None] & vx[:, None, :])[..., None]
        val = val.reshape(k, P, S, P, S, -1).sum(dim=(2, 4)) / float(S * S)
        outs.append(val.permute(0, 3, 1, 2))
    return torch.cat(outs, dim=0)


class _RoIAlignFn(torch.autograd.Function):
    """hip.roi_align / hip.roi_align_backward as one differentiable operation over f32 NCHW maps (any memory format); the RoIs get
    no gradient (torchvision's do not either)."""

    @staticmethod
    def forward(ctx, rois, levels, scales, P, S, *feats):
        nhwc = [f.detach().permute(0, 2, 3, 1).contiguous() for f in feats]
        ctx.save_for_backward(rois, levels)
        ctx.meta = (tuple(scales), P, S, [tuple(f.shape[1:3]) for f in nhwc], int(feats[0].shape[0]))
        return hip.roi_align(nhwc, scales, rois, levels, P, S)

    @staticmethod
    def backward(ctx, grad_out):
        rois, levels = ctx.saved_tensors
        scales, P, S, sizes, N = ctx.meta
        grads = hip.roi_align_backward(grad_out.to(torch.float32).contiguous(), sizes, scales, rois, levels, N, S)
        return (None, None, None, None, None) + tuple(g.permute(0, 3, 1, 2) for g in grads)


def multiscale_roi_align(feats, scales, rois, levels, output_size, sampling_ratio):
    """RoIAlign (aligned=False) of rois f32 [K,5] (image index, x1, y1, x2, y2), each from the map `levels[k]` of `feats`
    (NCHW maps of one batch, any memory format; `scales[l]`: image pixels -> pixels of map l) -> f32 [K,C,P,P]."""
    feats = list(feats)
    P, S = int(output_size), int(sampling_ratio)
    if S <= 0:
        raise NotImplementedError('roi_align: the adaptive sampling grid (sampling_ratio <= 0) is not built')
    rois = rois.to(torch.float32)
    # f32 maps that ask for a gradient: the kernel pair, or (switch off) autograd through the torch ops below.  bf16 maps keep
    # the inference kernel whatever they ask for: there is no bf16 backward.
    wants_grad = torch.is_grad_enabled() and any(f.requires_grad for f in feats) and all(f.dtype == torch.float32 for f in feats)
    if wants_grad and feats[0].is_cuda and hip.host_policy.roi_align_hip and hip.host_policy.roi_align_bwd_hip and feats[0].shape[1] % 8 == 0:
        return _RoIAlignFn.apply(rois.detach().contiguous(), levels.to(torch.int32).contiguous(), tuple(float(s) for s in scales), P, S, *feats)
    if feats[0].is_cuda and hip.host_policy.roi_align_hip and not wants_grad:
        if feats[0].shape[1] % 8:
            raise ValueError('roi_align: {} channels (the kernel takes multiples of 8)'.format(feats[0].shape[1]))
        dtype = torch.bfloat16 if feats[0].dtype == torch.bfloat16 else torch.float32
        nhwc = [f.to(dtype).permute(0, 2, 3, 1).contiguous() for f in feats]     # a view for channels_last maps
        return hip.roi_align(nhwc, [float(s) for s in scales], rois.contiguous(), levels.to(torch.int32).contiguous(), P, S)
    out = torch.zeros((rois.shape[0], feats[0].shape[1], P, P), dtype=torch.float32, device=rois.device)
    for l, (f, s) in enumerate(zip(feats, scales)):
        idx = torch.where(levels == l)[0]
        if idx.numel():
            out[idx] = _roi_align_level_torch(f, rois[idx], float(s), P, S)
    return out


def roi_align(input, boxes, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False):
    """torchvision.ops.roi_align for a square output and aligned=False.  boxes: Tensor [K,5] or a list of [k_i,4] per image."""
    if aligned:
        raise NotImplementedError('roi_align: aligned=True is not built (MultiScaleRoIAlign inside FasterRCNN uses aligned=False)')
    if isinstance(output_size, (tuple, list)):
        if output_size[0] != output_size[1]:
            raise NotImplementedError('roi_align: output_size must be square')
        output_size = output_size[0]
    if not isinstance(boxes, torch.Tensor):
        boxes = convert_to_roi_format(boxes)
    levels = torch.zeros(boxes.shape[0], dtype=torch.int32, device=boxes.device)
    return multiscale_roi_align([input], [spatial_scale], boxes, levels, output_size, sampling_ratio).to(input.dtype)


def convert_to_roi_format(boxes):
    concat = torch.cat(list(boxes), dim=0)
    ids = torch.cat([torch.full_like(b[:, :1], i) for i, b in enumerate(boxes)], dim=0)
    return torch.cat([ids, concat], dim=1)


class LevelMapper(object):
    """FPN paper eq. 1: the pyramid level of a box from its area (torchvision.ops.poolers.LevelMapper)."""

    def __init__(self, k_min, k_max, canonical_scale=224, canonical_level=4, eps=1e-6):
        self.k_min, self.k_max, self.s0, self.lvl0, self.eps = k_min, k_max, canonical_scale, canonical_level, eps

    def __call__(self, boxlists):
        s = torch.sqrt(torch.cat([(b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) for b in boxlists]))
        target = torch.floor(self.lvl0 + torch.log2(s / self.s0) + torch.tensor(self.eps, dtype=s.dtype))
        return (torch.clamp(target, min=self.k_min, max=self.k_max).to(torch.int64) - self.k_min).to(torch.int64)


class MultiScaleRoIAlign(nn.Module):
    """torchvision.ops.MultiScaleRoIAlign.  The feature maps are FILTERED BY NAME: the reference's configs name the pyramid
    '1', '2', '3', '4', 'pool' while FasterRCNN's default pooler asks for '0', '1', '2', '3', so only three maps (strides 4, 8, 16)
    reach it and large RoIs clamp to stride 16 -- the reference's behaviour, kept as it is."""

    def __init__(self, featmap_names, output_size, sampling_ratio, canonical_scale=224, canonical_level=4):
        super().__init__()
        if isinstance(output_size, int):
            output_size = (output_size, output_size)
        self.featmap_names = list(featmap_names)
        self.output_size = tuple(output_size)
        self.sampling_ratio = sampling_ratio
        self.canonical_scale, self.canonical_level = canonical_scale, canonical_level
        self.scales = None
        self.map_levels = None

    def setup_scales(self, features, image_shapes):
        max_h, max_w = max(s[0] for s in image_shapes), max(s[1] for s in image_shapes)
        self.scales = [2.0 ** float(round(math.log2(float(f.shape[-2]) / float(max_h)))) for f in features]
        assert all(2.0 ** float(round(math.log2(float(f.shape[-1]) / float(max_w)))) == s for f, s in zip(features, self.scales))
        k_min, k_max = -math.log2(self.scales[0]), -math.log2(self.scales[-1])
        self.map_levels = LevelMapper(int(k_min), int(k_max), self.canonical_scale, self.canonical_level)

    def filtered(self, x):
        feats = [v for k, v in x.items() if k in self.featmap_names]
        if not feats:
            raise ValueError('MultiScaleRoIAlign: none of the feature maps {} is named in {}'.format(list(x.keys()), self.featmap_names))
        return feats

    def forward(self, x, boxes, image_shapes):
        feats = self.filtered(x)
        self.setup_scales(feats, image_shapes)
        rois = convert_to_roi_format([b.to(torch.float32) for b in boxes])
        if len(feats) == 1:
            levels = torch.zeros(rois.shape[0], dtype=torch.int64, device=rois.device)
        else:
            levels = self.map_levels([b.to(torch.float32) for b in boxes])      # torch ops on every path
        if self.output_size[0] != self.output_size[1]:
            raise NotImplementedError('MultiScaleRoIAlign: output_size must be square')
        return multiscale_roi_align(feats, self.scales, rois, levels, self.output_size[0], self.sampling_ratio)


# ------------------------------------------------------------------------------------------------ anchors, RPN
class ImageList(object):
    def __init__(self, tensors, image_sizes):
        self.tensors = tensors
        self.image_sizes = image_sizes

    def to(self, device):
        return ImageList(self.tensors.to(device), self.image_sizes)


class AnchorGenerator(nn.Module):
    def __init__(self, sizes=((128, 256, 512),), aspect_ratios=((0.5, 1.0, 2.0),)):
        super().__init__()
        if not isinstance(sizes[0], (list, tuple)):
            sizes = tuple((s,) for s in sizes)
        if not isinstance(aspect_ratios[0], (list, tuple)):
            aspect_ratios = (aspect_ratios,) * len(sizes)
        self.sizes, self.aspect_ratios = sizes, aspect_ratios
        self.cell_anchors = [self.generate_anchors(s, a) for s, a in zip(sizes, aspect_ratios)]

    @staticmethod
    def generate_anchors(scales, aspect_ratios, dtype=torch.float32, device='cpu'):
        scales = torch.as_tensor(scales, dtype=dtype, device=device)
        h_ratios = torch.sqrt(torch.as_tensor(aspect_ratios, dtype=dtype, device=device))
        w_ratios = 1 / h_ratios
        ws, hs = (w_ratios[:, None] * scales[None, :]).view(-1), (h_ratios[:, None] * scales[None, :]).view(-1)
        return (torch.stack([-ws, -hs, ws, hs], dim=1) / 2).round()

    def num_anchors_per_location(self):
        return [len(s) * len(a) for s, a in zip(self.sizes, self.aspect_ratios)]

    def grid_anchors(self, grid_sizes, strides, dtype, device):
        if len(grid_sizes) != len(self.cell_anchors):
            raise ValueError('AnchorGenerator: {} feature maps for {} anchor sizes'.format(len(grid_sizes), len(self.cell_anchors)))
        anchors = []
        for (gh, gw), (sh, sw), base in zip(grid_sizes, strides, self.cell_anchors):
            shifts_x = torch.arange(0, gw, dtype=torch.int32, device=device) * sw
            shifts_y = torch.arange(0, gh, dtype=torch.int32, device=device) * sh
            shift_y, shift_x = torch.meshgrid(shifts_y, shifts_x, indexing='ij')
            shift_x, shift_y = shift_x.reshape(-1), shift_y.reshape(-1)
            shifts = torch.stack((shift_x, shift_y, shift_x, shift_y), dim=1)
            anchors.append((shifts.view(-1, 1, 4) + base.to(dtype=dtype, device=device).view(1, -1, 4)).reshape(-1, 4))   # (y, x, anchor)
        return anchors

    def forward(self, image_list, feature_maps):
        grid_sizes = [tuple(f.shape[-2:]) for f in feature_maps]
        image_size = image_list.tensors.shape[-2:]
        strides = [(image_size[0] // g[0], image_size[1] // g[1]) for g in grid_sizes]
        per_level = self.grid_anchors(grid_sizes, strides, torch.float32, feature_maps[0].device)
        return [torch.cat(per_level) for _ in image_list.image_sizes]


class RPNHead(nn.Module):
    """3x3 conv + ReLU, then 1x1 objectness (A channels) and 1x1 box deltas (4A).  Keys `conv.0.0.*` (torchvision 0.13+: the conv
    sits in a Conv2dNormActivation inside a Sequential); the earlier `conv.*` is accepted on load."""

    def __init__(self, in_channels, num_anchors, conv_depth=1):
        super().__init__()
        self.conv = nn.Sequential(*[nn.Sequential(nn.Conv2d(in_channels, in_channels, 3, padding=1), nn.ReLU(inplace=True))
                                    for _ in range(conv_depth)])
        self.cls_logits = nn.Conv2d(in_channels, num_anchors, 1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors * 4, 1)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.01)
                nn.init.constant_(m.bias, 0)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for t in ('weight', 'bias'):
            old, new = '{}conv.{}'.format(prefix, t), '{}conv.0.0.{}'.format(prefix, t)
            if old in state_dict:
                state_dict[new] = state_dict.pop(old)
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def forward(self, x):
        dtype = self.cls_logits.weight.dtype
        logits, bbox_reg = [], []
        for feature in x:
            t = self.conv(feature.to(dtype))
            logits.append(self.cls_logits(t))
            bbox_reg.append(self.bbox_pred(t))
        return logits, bbox_reg


def permute_and_flatten(layer, N, A, C, H, W):
    return layer.view(N, -1, C, H, W).permute(0, 3, 4, 1, 2).reshape(N, -1, C)      # (N,A,C,H,W) -> (N,H,W,A,C)


def concat_box_prediction_layers(box_cls, box_regression):
    cls_flat, reg_flat = [], []
    for cls_l, reg_l in zip(box_cls, box_regression):
        N, AxC, H, W = cls_l.shape
        A = reg_l.shape[1] // 4
        cls_flat.append(permute_and_flatten(cls_l, N, A, AxC // A, H, W))
        reg_flat.append(permute_and_flatten(reg_l, N, A, 4, H, W))
    return torch.cat(cls_flat, dim=1).flatten(0, -2), torch.cat(reg_flat, dim=1).reshape(-1, 4)


_TRAINING_OFF = ('{}: the training path is off for this module -- the proposal matcher, the balanced positive / negative samplers and '
                 'the classification / box-regression losses run only behind `detection.enable_training(model)` (a '
                 "`forward_proc: 'forward_batch_target'` student gets it from `training.DistillationStage`); a module that was only "
                 'put into train() keeps raising, as it always has')


def enable_training(model, enabled=True):
    """Switch the loss path of every `RegionProposalNetwork` and `RoIHeads` inside `model` on (or off) -> model.  The path is an
    opt-in per module: without it a module in training mode raises NotImplementedError, the behaviour from before the path was built."""
    for m in model.modules():
        if isinstance(m, (RegionProposalNetwork, RoIHeads)):
            m.training_enabled = bool(enabled)
    return model


class RegionProposalNetwork(nn.Module):
    training_enabled = False      # see `enable_training`

    def __init__(self, anchor_generator, head, fg_iou_thresh=0.7, bg_iou_thresh=0.3, batch_size_per_image=256, positive_fraction=0.5,
                 pre_nms_top_n=None, post_nms_top_n=None, nms_thresh=0.7, score_thresh=0.0):
        super().__init__()
        self.anchor_generator = anchor_generator
        self.head = head
        self.box_coder = BoxCoder(weights=(1.0, 1.0, 1.0, 1.0))
        self.fg_iou_thresh, self.bg_iou_thresh = fg_iou_thresh, bg_iou_thresh
        self.batch_size_per_image, self.positive_fraction = batch_size_per_image, positive_fraction
        self._pre_nms_top_n = pre_nms_top_n or dict(training=2000, testing=1000)
        self._post_nms_top_n = post_nms_top_n or dict(training=2000, testing=1000)
        self.nms_thresh = nms_thresh
        self.score_thresh = score_thresh
        self.min_size = 1e-3

    def pre_nms_top_n(self):
        return self._pre_nms_top_n['training' if self.training else 'testing']

    def post_nms_top_n(self):
        return self._post_nms_top_n['training' if self.training else 'testing']

    def _get_top_n_idx(self, objectness, num_anchors_per_level):
        r, offset = [], 0
        for ob in objectness.split(num_anchors_per_level, 1):
            n = ob.shape[1]
            r.append(ob.topk(min(self.pre_nms_top_n(), n), dim=1)[1] + offset)
            offset += n
        return torch.cat(r, dim=1)

    def filter_proposals(self, proposals, objectness, image_shapes, num_anchors_per_level):
        num_images = proposals.shape[0]
        device = proposals.device
        objectness = objectness.detach().reshape(num_images, -1)
        levels = torch.cat([torch.full((n,), idx, dtype=torch.int64, device=device) for idx, n in enumerate(num_anchors_per_level)], 0)
        levels = levels.reshape(1, -1).expand_as(objectness)
        top_n_idx = self._get_top_n_idx(objectness, num_anchors_per_level)       # chosen on the logits
        batch_idx = torch.arange(num_images, device=device)[:, None]
        objectness, levels, proposals = objectness[batch_idx, top_n_idx], levels[batch_idx, top_n_idx], proposals[batch_idx, top_n_idx]
        objectness_prob = torch.sigmoid(objectness)
        final_boxes, final_scores = [], []
        for boxes, scores, lvl, img_shape in zip(proposals, objectness_prob, levels, image_shapes):
            boxes = clip_boxes_to_image(boxes, img_shape)
            keep = remove_small_boxes(boxes, self.min_size)
            boxes, scores, lvl = boxes[keep], scores[keep], lvl[keep]
            keep = torch.where(scores >= self.score_thresh)[0]
            boxes, scores, lvl = boxes[keep], scores[keep], lvl[keep]
            keep = batched_nms(boxes, scores, lvl, self.nms_thresh)[:self.post_nms_top_n()]
            final_boxes.append(boxes[keep])
            final_scores.append(scores[keep])
        return final_boxes, final_scores

    def _proposals_on_kernel(self, objectness, pred_bbox_deltas, anchors, image_shapes):
        """The whole batch on `hip.rpn_proposals` (three launches on the head's per-level outputs as they stand -- no concat, no
        decode of every anchor -- and one read-back of the counts) -> the per-image list of proposals, or None where that path does
        not apply: CPU tensors, `hip.host_policy.rpn_post_hip` or `nms_hip` off, another dtype than f32, an anchor generator other
        than this module's `AnchorGenerator` (whose images share one anchor set by construction), or dimensions outside the
        kernel's caps.  The caller then runs `filter_proposals`."""
        if not (len(objectness) > 0 and objectness[0].is_cuda and hip.host_policy.rpn_post_hip and hip.host_policy.nms_hip):     # (nms_hip off: the tail on torch ops, A/B)
            return None
        if type(self.anchor_generator) is not AnchorGenerator or len(anchors) == 0 or len(anchors) != len(image_shapes):
            return None
        maps = list(objectness) + list(pred_bbox_deltas)
        if len(objectness) != len(pred_bbox_deltas) or any(t.dtype != torch.float32 or t.device != maps[0].device for t in maps + [anchors[0]]):
            return None
        if any(t.dim() != 4 for t in maps) or anchors[0].dim() != 2:
            return None
        N, K, P = len(anchors), int(self.pre_nms_top_n()), int(self.post_nms_top_n())
        shapes = [tuple(int(v) for v in o.shape[1:]) for o in objectness]
        if (any(int(o.shape[0]) != N or tuple(d.shape) != (N, 4 * s[0], s[1], s[2]) for o, d, s in zip(objectness, pred_bbox_deltas, shapes))
                or not hip.rpn_proposals_in_range(shapes, N, K, P) or int(anchors[0].shape[0]) != sum(a * h * w for a, h, w in shapes)):
            return None
        res = hip.rpn_proposals([o.detach().contiguous() for o in objectness], [d.detach().contiguous() for d in pred_bbox_deltas],
                                anchors[0].contiguous(), [(int(h), int(w)) for h, w in image_shapes], K, P, self.nms_thresh,
                                self.score_thresh, self.min_size, self.box_coder.weights, self.box_coder.bbox_xform_clip)
        return [res.boxes[i, :k] for i, k in enumerate(res.count.cpu().tolist())]

    def assign_targets_to_anchors(self, anchors, targets):
        """-> (labels f32 [A] per image: 1 matched, 0 background, -1 between the thresholds; the matched gt box of every anchor).
        Thresholds fg / bg (0.7 / 0.3) with low-quality matches on; an image without gt boxes: all-zero labels and boxes."""
        gt_boxes = [t['boxes'] for t in targets]
        matched = match_boxes(gt_boxes, anchors, self.fg_iou_thresh, self.bg_iou_thresh, True)
        labels, matched_gt_boxes = [], []
        for anchors_per_image, gt, m in zip(anchors, gt_boxes, matched):
            if gt.numel() == 0:
                matched_gt_boxes.append(torch.zeros_like(anchors_per_image))
                labels.append(torch.zeros((anchors_per_image.shape[0],), dtype=torch.float32, device=anchors_per_image.device))
                continue
            matched_gt_boxes.append(gt.to(anchors_per_image.dtype)[m.clamp(min=0)])
            lab = (m >= 0).to(torch.float32)
            lab = torch.where(m == Matcher.BELOW_LOW_THRESHOLD, torch.zeros_like(lab), lab)
            lab = torch.where(m == Matcher.BETWEEN_THRESHOLDS, torch.full_like(lab, -1.0), lab)
            labels.append(lab)
        return labels, matched_gt_boxes

    def compute_loss(self, objectness, pred_bbox_deltas, labels, regression_targets):
        """BCE-with-logits on the sampled anchors; smooth-L1 (beta 1/9) summed over the sampled positives / the number sampled"""
        sampled_pos, sampled_neg = BalancedPositiveNegativeSampler(self.batch_size_per_image, self.positive_fraction)(labels)
        sampled_pos = torch.where(torch.cat(sampled_pos, dim=0))[0]
        sampled_neg = torch.where(torch.cat(sampled_neg, dim=0))[0]
        sampled = torch.cat([sampled_pos, sampled_neg], dim=0)
        objectness = objectness.flatten()
        labels, regression_targets = torch.cat(labels, dim=0), torch.cat(regression_targets, dim=0)
        box_loss = smooth_l1_loss(pred_bbox_deltas[sampled_pos], regression_targets[sampled_pos], beta=1.0 / 9) / sampled.numel()
        objectness_loss = F.binary_cross_entropy_with_logits(objectness[sampled], labels[sampled])
        return objectness_loss, box_loss

    def forward(self, images, features, targets=None):
        if self.training:
            if targets is None:
                raise ValueError('targets should not be None in training mode')
            if not self.training_enabled:
                raise NotImplementedError(_TRAINING_OFF.format('RegionProposalNetwork'))
        features = list(features.values())
        objectness, pred_bbox_deltas = self.head(features)
        anchors = self.anchor_generator(images, features)
        num_images = len(anchors)
        num_anchors_per_level = [o[0].numel() for o in objectness]
        boxes = self._proposals_on_kernel(objectness, pred_bbox_deltas, anchors, images.image_sizes)
        if boxes is None or self.training:       # (the loss reads the concatenation)
            objectness, pred_bbox_deltas = concat_box_prediction_layers(objectness, pred_bbox_deltas)
        if boxes is None:
            proposals = self.box_coder.decode(pred_bbox_deltas.detach().float(), anchors).view(num_images, -1, 4)
            boxes, _ = self.filter_proposals(proposals, objectness.float(), images.image_sizes, num_anchors_per_level)
        losses = {}
        if self.training:
            labels, matched_gt_boxes = self.assign_targets_to_anchors(anchors, targets)
            regression_targets = self.box_coder.encode(matched_gt_boxes, anchors)
            loss_objectness, loss_rpn_box_reg = self.compute_loss(objectness.float(), pred_bbox_deltas.float(), labels, regression_targets)
            losses = {'loss_objectness': loss_objectness, 'loss_rpn_box_reg': loss_rpn_box_reg}
        return boxes, losses


# ------------------------------------------------------------------------------------------------ box head, RoI heads
class TwoMLPHead(nn.Module):
    def __init__(self, in_channels, representation_size):
        super().__init__()
        self.fc6 = nn.Linear(in_channels, representation_size)
        self.fc7 = nn.Linear(representation_size, representation_size)

    def forward(self, x):
        x = x.flatten(start_dim=1).to(self.fc6.weight.dtype)
        return F.relu(self.fc7(F.relu(self.fc6(x))))


class FastRCNNPredictor(nn.Module):
    def __init__(self, in_channels, num_classes):
        super().__init__()
        self.cls_score = nn.Linear(in_channels, num_classes)
        self.bbox_pred = nn.Linear(in_channels, num_classes * 4)

    def forward(self, x):
        if x.dim() == 4 and list(x.shape[2:]) != [1, 1]:
            raise ValueError('FastRCNNPredictor: expected the last two dimensions to be [1,1], got {}'.format(list(x.shape[2:])))
        x = x.flatten(start_dim=1)
        return self.cls_score(x), self.bbox_pred(x)


class RoIHeads(nn.Module):
    training_enabled = False      # see `enable_training`

    def __init__(self, box_roi_pool, box_head, box_predictor, fg_iou_thresh=0.5, bg_iou_thresh=0.5, batch_size_per_image=512,
                 positive_fraction=0.25, bbox_reg_weights=None, score_thresh=0.05, nms_thresh=0.5, detections_per_img=100):
        super().__init__()
        self.box_roi_pool, self.box_head, self.box_predictor = box_roi_pool, box_head, box_predictor
        self.fg_iou_thresh, self.bg_iou_thresh = fg_iou_thresh, bg_iou_thresh
        self.batch_size_per_image, self.positive_fraction = batch_size_per_image, positive_fraction
        self.box_coder = BoxCoder((10.0, 10.0, 5.0, 5.0) if bbox_reg_weights is None else bbox_reg_weights)
        self.score_thresh, self.nms_thresh, self.detections_per_img = score_thresh, nms_thresh, detections_per_img

    def _postprocess_on_kernel(self, class_logits, box_regression, proposals, image_shapes):
        """The whole batch on `hip.det_postprocess` (three launches, one read-back of the counts and the status words) -> the lists
        of `postprocess_detections`, or None where that path does not apply -- CPU tensors, `hip.host_policy.det_post_hip` or
        `nms_hip` off, another dtype than f32, a class count or `detections_per_img` outside the kernel's range -- or where an image exceeds one of
        the kernel's candidate caps (a non-zero status): the caller then runs the loop below."""
        if not (class_logits.is_cuda and hip.host_policy.det_post_hip and hip.host_policy.nms_hip):     # (nms_hip off: the tail on torch ops, A/B)
            return None
        tensors = [class_logits, box_regression] + list(proposals)
        if any(t.dtype != torch.float32 or t.device != class_logits.device for t in tensors) or class_logits.dim() != 2:
            return None
        C, D, n = int(class_logits.shape[-1]), int(self.detections_per_img), len(proposals)
        if not (2 <= C <= hip.DETPOST_MAX_CLASSES and 1 <= D <= hip.DETPOST_MAX_DET and 1 <= n == len(image_shapes) and n <= 65535
                and int(class_logits.shape[0]) * (C - 1) < 2 ** 31):
            return None
        res = hip.det_postprocess(class_logits.detach().contiguous(), box_regression.detach().contiguous(),
                                  torch.cat(list(proposals), dim=0).detach().contiguous(), [int(p.shape[0]) for p in proposals],
                                  [(int(h), int(w)) for h, w in image_shapes], self.box_coder.weights, self.box_coder.bbox_xform_clip,
                                  self.score_thresh, 1e-2, self.nms_thresh, D)
        counts, status = res.count_status.cpu().tolist()
        if any(status):
            return None
        return ([res.boxes[i, :k] for i, k in enumerate(counts)], [res.scores[i, :k] for i, k in enumerate(counts)],
                [res.labels[i, :k] for i, k in enumerate(counts)])

    def postprocess_detections(self, class_logits, box_regression, proposals, image_shapes):
        on_kernel = self._postprocess_on_kernel(class_logits, box_regression, proposals, image_shapes)
        if on_kernel is not None:
            return on_kernel
        device = class_logits.device
        num_classes = class_logits.shape[-1]
        boxes_per_image = [b.shape[0] for b in proposals]
        pred_boxes = self.box_coder.decode(box_regression, proposals)
        pred_scores = F.softmax(class_logits, -1)
        all_boxes, all_scores, all_labels = [], [], []
        for boxes, scores, image_shape in zip(pred_boxes.split(boxes_per_image, 0), pred_scores.split(boxes_per_image, 0), image_shapes):
            boxes = clip_boxes_to_image(boxes, image_shape)
            labels = torch.arange(num_classes, device=device).view(1, -1).expand_as(scores)
            boxes, scores, labels = boxes[:, 1:].reshape(-1, 4), scores[:, 1:].reshape(-1), labels[:, 1:].reshape(-1)   # no background
            inds = torch.where(scores > self.score_thresh)[0]
            boxes, scores, labels = boxes[inds], scores[inds], labels[inds]
            keep = remove_small_boxes(boxes, min_size=1e-2)
            boxes, scores, labels = boxes[keep], scores[keep], labels[keep]
            keep = batched_nms(boxes, scores, labels, self.nms_thresh)[:self.detections_per_img]
            all_boxes.append(boxes[keep])
            all_scores.append(scores[keep])
            all_labels.append(labels[keep])
        return all_boxes, all_scores, all_labels

    @staticmethod
    def check_targets(targets):
        if targets is None:
            raise ValueError('targets should not be None in training mode')
        if not all('boxes' in t for t in targets):
            raise ValueError('Every element of targets should have a boxes key')
        if not all('labels' in t for t in targets):
            raise ValueError('Every element of targets should have a labels key')

    @staticmethod
    def add_gt_proposals(proposals, gt_boxes):
        return [torch.cat((p, g)) for p, g in zip(proposals, gt_boxes)]

    def assign_targets_to_proposals(self, proposals, gt_boxes, gt_labels):
        """-> (matched gt index clamped at 0, labels int64: the gt label, 0 background, -1 ignored) per image; fg / bg thresholds
        (0.5 / 0.5) without low-quality matches"""
        matched = match_boxes(gt_boxes, proposals, self.fg_iou_thresh, self.bg_iou_thresh, False)
        matched_idxs, labels = [], []
        for m, labels_in_image in zip(matched, gt_labels):
            clamped = m.clamp(min=0)
            if labels_in_image.numel() == 0:
                lab = torch.zeros_like(clamped)
            else:
                lab = labels_in_image[clamped].to(torch.int64)
                lab = torch.where(m == Matcher.BELOW_LOW_THRESHOLD, torch.zeros_like(lab), lab)
                lab = torch.where(m == Matcher.BETWEEN_THRESHOLDS, torch.full_like(lab, -1), lab)
            matched_idxs.append(clamped)
            labels.append(lab)
        return matched_idxs, labels

    def subsample(self, labels):
        sampled_pos, sampled_neg = BalancedPositiveNegativeSampler(self.batch_size_per_image, self.positive_fraction)(labels)
        return [torch.where(p | n)[0] for p, n in zip(sampled_pos, sampled_neg)]

    def select_training_samples(self, proposals, targets):
        self.check_targets(targets)
        dtype = proposals[0].dtype
        gt_boxes = [t['boxes'].to(dtype).reshape(-1, 4) for t in targets]
        gt_labels = [t['labels'] for t in targets]
        proposals = self.add_gt_proposals(proposals, gt_boxes)
        matched_idxs, labels = self.assign_targets_to_proposals(proposals, gt_boxes, gt_labels)
        sampled_inds = self.subsample(labels)
        matched_gt_boxes = []
        for i, inds in enumerate(sampled_inds):
            proposals[i], labels[i], matched_idxs[i] = proposals[i][inds], labels[i][inds], matched_idxs[i][inds]
            gt = gt_boxes[i] if gt_boxes[i].numel() else torch.zeros((1, 4), dtype=dtype, device=proposals[i].device)
            matched_gt_boxes.append(gt[matched_idxs[i]])
        regression_targets = self.box_coder.encode(matched_gt_boxes, proposals)
        return proposals, matched_idxs, labels, regression_targets

    @staticmethod
    def fastrcnn_loss(class_logits, box_regression, labels, regression_targets):
        """cross entropy; smooth-L1 (beta 1/9) on the positive rows' own class, summed / the number of sampled RoIs"""
        labels, regression_targets = torch.cat(labels, dim=0), torch.cat(regression_targets, dim=0)
        classification_loss = F.cross_entropy(class_logits, labels)
        pos = torch.where(labels > 0)[0]
        box_regression = box_regression.reshape(class_logits.shape[0], box_regression.size(-1) // 4, 4)
        box_loss = smooth_l1_loss(box_regression[pos, labels[pos]], regression_targets[pos], beta=1.0 / 9) / labels.numel()
        return classification_loss, box_loss

    def forward(self, features, proposals, image_shapes, targets=None):
        if self.training:
            if targets is None:
                raise ValueError('targets should not be None in training mode')
            if not self.training_enabled:
                raise NotImplementedError(_TRAINING_OFF.format('RoIHeads'))
            proposals, _, labels, regression_targets = self.select_training_samples(proposals, targets)
            box_features = self.box_head(self.box_roi_pool(features, proposals, image_shapes))
            class_logits, box_regression = self.box_predictor(box_features)
            loss_classifier, loss_box_reg = self.fastrcnn_loss(class_logits.float(), box_regression.float(), labels, regression_targets)
            return [], {'loss_classifier': loss_classifier, 'loss_box_reg': loss_box_reg}
        box_features = self.box_head(self.box_roi_pool(features, proposals, image_shapes))
        class_logits, box_regression = self.box_predictor(box_features)
        boxes, scores, labels = self.postprocess_detections(class_logits.float(), box_regression.float(), proposals, image_shapes)
        return [{'boxes': b, 'labels': l, 'scores': s} for b, l, s in zip(boxes, labels, scores)], {}


# ------------------------------------------------------------------------------------------------ transform, model
def resize_boxes(boxes, original_size, new_size):
    ratio_h, ratio_w = [torch.tensor(s, dtype=torch.float32, device=boxes.device) / torch.tensor(o, dtype=torch.float32, device=boxes.device)
                        for s, o in zip(new_size, original_size)]
    xmin, ymin, xmax, ymax = boxes.unbind(1)
    return torch.stack((xmin * ratio_w, ymin * ratio_h, xmax * ratio_w, ymax * ratio_h), dim=1)


def original_sizes(images):
    """[(h, w)] of a list of [C,H,W] images or of a planned batch (`transforms.DeferredDetBatch.sizes`)"""
    if isinstance(images, DeferredDetBatch):
        return [tuple(size) for size in images.sizes]
    return [tuple(img.shape[-2:]) for img in images]


class GeneralizedRCNNTransform(nn.Module):
    """Normalise, resize so that the shorter side is min_size unless the longer would pass max_size, zero-pad the batch to a
    multiple of `size_divisible`; `postprocess` maps the detections back to each image's own size."""

    def __init__(self, min_size, max_size, image_mean, image_std, size_divisible=32, fixed_size=None, **kwargs):
        super().__init__()
        self.min_size = tuple(min_size) if isinstance(min_size, (list, tuple)) else (min_size,)
        self.max_size = max_size
        self.image_mean, self.image_std = image_mean, image_std
        self.size_divisible = size_divisible
        self.fixed_size = fixed_size
        self._skip_resize = kwargs.pop('_skip_resize', False)

    def normalize(self, image):
        if not image.is_floating_point():
            raise TypeError('Expected input images to be of floating type (in range [0, 1]), but found type {}'.format(image.dtype))
        mean = torch.as_tensor(self.image_mean, dtype=image.dtype, device=image.device)
        std = torch.as_tensor(self.image_std, dtype=image.dtype, device=image.device)
        return (image - mean[:, None, None]) / std[:, None, None]

    def resized_size(self, h, w):
        """the size `resize` produces from an h x w image in eval mode: floor(side * scale), as F.interpolate recomputes it"""
        if self.fixed_size is not None:
            return self.fixed_size[1], self.fixed_size[0]
        scale = min(float(self.min_size[-1]) / min(h, w), float(self.max_size) / max(h, w))
        return int(math.floor(h * scale)), int(math.floor(w * scale))

    def resize(self, image, target=None):
        h, w = image.shape[-2:]
        if self.training and self._skip_resize:
            return image, target
        if self.fixed_size is not None:
            image = F.interpolate(image[None], size=[self.fixed_size[1], self.fixed_size[0]], mode='bilinear', align_corners=False)[0]
        else:
            scale = min(float(self.min_size[-1]) / min(h, w), float(self.max_size) / max(h, w))
            image = F.interpolate(image[None], scale_factor=scale, mode='bilinear', recompute_scale_factor=True, align_corners=False)[0]
        if target is not None and 'boxes' in target:
            target = dict(target, boxes=resize_boxes(target['boxes'], (h, w), image.shape[-2:]))
        return image, target

    def batch_images(self, images):
        stride = float(self.size_divisible)
        max_h, max_w = max(i.shape[-2] for i in images), max(i.shape[-1] for i in images)
        max_h, max_w = int(math.ceil(max_h / stride) * stride), int(math.ceil(max_w / stride) * stride)
        batched = images[0].new_full((len(images), images[0].shape[0], max_h, max_w), 0)
        for i, img in enumerate(images):
            batched[i, :, :img.shape[1], :img.shape[2]].copy_(img)
        return batched

    def _det_input_plan(self, batch):
        """True when a planned batch takes the kernel path (`DeferredDetBatch.transformed`: one copy up of the source bytes and one
        sc2_det_input launch): a HIP device, `hip.host_policy.det_input_hip` on, no fixed size, the resize not skipped, three
        channels' statistics and every side within the kernel's cap.  Decided before anything is launched."""
        if batch.device.type != 'cuda' or not hip.host_policy.det_input_hip or self.fixed_size is not None:
            return False
        if (self.training and self._skip_resize) or len(batch) == 0 or len(self.image_mean) != 3 or len(self.image_std) != 3:
            return False
        if any(float(v) == 0.0 for v in self.image_std) or batch.buf.numel() > 0x7FFFFFFF:
            return False
        for h, w in batch.sizes:
            oh, ow = self.resized_size(h, w)
            if max(h, w, oh, ow) > hip.JPEG_IMAGE_MAX_SIDE or min(h, w, oh, ow) < 1:
                return False
        return True

    def _forward_deferred(self, batch, targets):
        """a `transforms.DeferredDetBatch` as `images`: the same ImageList and targets as `forward(batch.tensors(device), targets)`"""
        if not self._det_input_plan(batch):
            return self.forward(batch.tensors(batch.device), targets)
        targets = [dict(t) for t in targets] if targets is not None else None
        batched, image_sizes = batch.transformed(self, batch.device)      # shared with every transform of equal parameters: read-only
        if targets is not None:
            for i, (size, new_size) in enumerate(zip(batch.sizes, image_sizes)):
                if 'boxes' in targets[i]:
                    targets[i] = dict(targets[i], boxes=resize_boxes(targets[i]['boxes'], size, new_size))
        return ImageList(batched, list(image_sizes)), targets

    def forward(self, images, targets=None):
        if isinstance(images, DeferredDetBatch):
            return self._forward_deferred(images, targets)
        images = [img for img in images]
        targets = [dict(t) for t in targets] if targets is not None else None
        for i, image in enumerate(images):
            if image.dim() != 3:
                raise ValueError('images is expected to be a list of 3d tensors of shape [C, H, W], got {}'.format(tuple(image.shape)))
            image, t = self.resize(self.normalize(image), targets[i] if targets is not None else None)
            images[i] = image
            if targets is not None:
                targets[i] = t
        image_sizes = [(int(img.shape[-2]), int(img.shape[-1])) for img in images]
        return ImageList(self.batch_images(images), image_sizes), targets

    def postprocess(self, result, image_shapes, original_image_sizes):
        if self.training:
            return result
        for i, (pred, im_s, o_im_s) in enumerate(zip(result, image_shapes, original_image_sizes)):
            result[i]['boxes'] = resize_boxes(pred['boxes'], im_s, o_im_s)
        return result


class RCNNTransformWithCompression(GeneralizedRCNNTransform, AnalyzableModule):
    """The R-CNN transform with a codec (or a compression model) between resize and normalise
    (sc2bench/models/detection/transform.py): per image resize -> compress -> normalise, then the zero-padded batch.  The file size
    (codec) or the compressed object (model) of every image goes to the analyzers in eval mode.

    `forward` has two forms with one result.  The HOST path is the reference's loop and is always available.  The KERNEL path
    (`_kernel_plan`: eval mode, `hip.host_policy.rcnn_input_hip` and `jpeg_image_hip` on, no compression model, no pre / post
    transform, a size-reporting `PILImageModule` with plain JPEG, 3-channel float32 device images whose sides stay within the
    codec's limit) runs `hip.rcnn_resize_u8` -> `hip.jpeg_image_codec` -> `hip.rcnn_normalize_pad` per image straight into the
    batch tensor, and reads the file sizes and the status words of all images back ONCE behind the last launch; an image whose
    status is set (a NaN or a value outside [0, 1], where `mul(255).byte()` wraps) is redone on the host path."""

    def __init__(self, transform, device, codec_encoder_decoder, analyzer_configs, analyzes_after_compress=False,
                 compression_model=None, uses_cpu4compression_model=False, pre_transform=None, post_transform=None,
                 adaptive_pad_kwargs=None):
        GeneralizedRCNNTransform.__init__(self, transform.min_size, transform.max_size, transform.image_mean, transform.image_std)
        AnalyzableModule.__init__(self, analyzer_configs)
        self.device = device
        self.codec_encoder_decoder = codec_encoder_decoder
        self.analyzes_after_compress = analyzes_after_compress
        self.pre_transform = pre_transform
        self.post_transform = post_transform
        if uses_cpu4compression_model and compression_model is not None:
            compression_model = compression_model.cpu()
        self.compression_model = compression_model
        self.uses_cpu4compression_model = uses_cpu4compression_model
        self.adaptive_pad = AdaptivePad(**adaptive_pad_kwargs) if isinstance(adaptive_pad_kwargs, dict) else None

    def compress_by_codec(self, org_img):
        pil_img, file_size = self.codec_encoder_decoder(to_pil_image(org_img))
        if not self.training:
            self.analyze(file_size)
        return to_tensor(pil_img).to(org_img.device)

    def compress_by_model(self, org_img):
        org_img = org_img.unsqueeze(0)
        org_height, org_width = None, None
        if self.adaptive_pad is not None:
            org_height, org_width = org_img.shape[-2:]
            org_img = self.adaptive_pad(org_img)
        compressed_obj = self.compression_model.compress(org_img)
        if not self.training and self.analyzes_after_compress:
            self.analyze(compressed_obj if org_height is None or org_width is None else (compressed_obj, org_height, org_width))
        decompressed = self.compression_model.decompress(**compressed_obj)['x_hat']
        if org_height is not None and org_width is not None:
            decompressed = decompressed[..., :org_height, :org_width]
        return decompressed.squeeze(0)

    def compress(self, org_img):
        if self.pre_transform is not None:
            org_img = self.pre_transform(org_img)
        org_device = org_img.device
        if self.uses_cpu4compression_model:
            org_img = org_img.cpu()
        org_img = self.compress_by_codec(org_img) if self.compression_model is None else self.compress_by_model(org_img)
        if self.uses_cpu4compression_model:
            org_img = org_img.to(org_device)
        if self.post_transform is not None:
            org_img = self.post_transform(org_img)
        return org_img

    def _host_image(self, image, target):
        """one image of the host path: -> (resized, compressed, normalised image, target with resized boxes)"""
        image, target = self.resize(image, target)
        shape_before_compression = image.shape
        image = self.compress(image)
        assert image.shape == shape_before_compression, \
            'Compression should not change tensor shape {} -> {}'.format(shape_before_compression, image.shape)
        return self.normalize(image), target

    def _kernel_plan(self, images):
        """(JPEG quality, [(oh, ow) of every image]) when this list takes the kernel path, else None.  Decided before anything is
        launched: the path is one for the whole list."""
        if self.training or not (hip.host_policy.rcnn_input_hip and hip.host_policy.jpeg_image_hip):
            return None
        if self.compression_model is not None or self.pre_transform is not None or self.post_transform is not None:
            return None
        if self.fixed_size is not None or len(images) == 0:
            return None
        codec = self.codec_encoder_decoder
        if isinstance(codec, Compose) and len(codec.transforms) == 1:
            codec = codec.transforms[0]
        if not isinstance(codec, PILImageModule) or not codec.returns_file_size:
            return None
        quality = codec._jpeg_quality()
        if quality is None:
            return None
        sizes = []
        for image in images:
            if not (isinstance(image, torch.Tensor) and image.is_cuda and image.dtype == torch.float32 and image.dim() == 3 and
                    image.shape[0] == 3 and image.device == images[0].device and min(image.shape[-2:]) >= 1):
                return None
            oh, ow = self.resized_size(int(image.shape[-2]), int(image.shape[-1]))
            if max(oh, ow, int(image.shape[-2]), int(image.shape[-1])) > hip.JPEG_IMAGE_MAX_SIDE or min(oh, ow) < 1:
                return None
            sizes.append((oh, ow))
        return quality, sizes

    def _forward_kernels(self, images, targets, quality, sizes):
        from . import jpeg_format
        for oh, ow in set(sizes):      # (the kernel counts whole files; the header length it adds is the one Pillow writes)
            if jpeg_format.checked_header_bytes('RGB', oh, ow, quality) != hip.JPEG_HEADER_BYTES[hip.JPEG_RGB]:
                raise hip.Sc2Error('jpeg header of {} bytes expected for mode RGB'.format(hip.JPEG_HEADER_BYTES[hip.JPEG_RGB]))
        dev, n = images[0].device, len(images)
        stride = float(self.size_divisible)
        max_h = int(math.ceil(max(s[0] for s in sizes) / stride) * stride)
        max_w = int(math.ceil(max(s[1] for s in sizes) / stride) * stride)
        batched = torch.empty((n, 3, max_h, max_w), dtype=torch.float32, device=dev)      # every element is written by the kernel
        status = torch.zeros((n,), dtype=torch.int32, device=dev)
        file_sizes = []
        for i, (image, (oh, ow)) in enumerate(zip(images, sizes)):
            pixels, _ = hip.rcnn_resize_u8(image, oh, ow, status=status[i:i + 1])
            coded = hip.jpeg_image_codec(pixels.unsqueeze(0), quality)
            file_sizes.append(coded.sizes)
            hip.rcnn_normalize_pad(coded.recon[0], self.image_mean, self.image_std, batched[i])
            if targets is not None and 'boxes' in targets[i]:
                targets[i] = dict(targets[i], boxes=resize_boxes(targets[i]['boxes'], tuple(image.shape[-2:]), (oh, ow)))
        back = torch.cat(file_sizes + [status]).cpu().tolist()      # the one read-back of the list
        for i, (file_size, flagged) in enumerate(zip(back[:n], back[n:])):      # analysed in image order
            if flagged:      # out of [0, 1]: what the host computes there (the bytes wrap) is the result
                image, _ = self._host_image(images[i], None)
                batched[i].zero_()
                batched[i, :, :image.shape[-2], :image.shape[-1]].copy_(image)
            else:
                self.analyze(file_size)
        return ImageList(batched, [(int(oh), int(ow)) for oh, ow in sizes]), targets

    def forward(self, images, targets=None):
        if isinstance(images, DeferredDetBatch):      # a planned batch: the codec works on the host chain's tensors
            images = images.tensors(images.device)
        images = [img for img in images]
        targets = [dict(t) for t in targets] if targets is not None else None
        for image in images:
            if image.dim() != 3:
                raise ValueError('images is expected to be a list of 3d tensors of shape [C, H, W], got {}'.format(tuple(image.shape)))
        plan = self._kernel_plan(images)
        if plan is not None:
            return self._forward_kernels(images, targets, *plan)
        for i, image in enumerate(images):
            image, target = self._host_image(image, targets[i] if targets is not None else None)
            images[i] = image
            if targets is not None and target is not None:
                targets[i] = target
        image_sizes = [(int(img.shape[-2]), int(img.shape[-1])) for img in images]
        return ImageList(self.batch_images(images), image_sizes), targets


class FasterRCNN(nn.Module):
    """torchvision.models.detection.FasterRCNN under its keyword names; `transform`, `backbone`, `rpn`, `roi_heads` are the
    attributes `dense.BaseRCNN` takes over."""

    def __init__(self, backbone, num_classes=None, min_size=800, max_size=1333, image_mean=None, image_std=None,
                 rpn_anchor_generator=None, rpn_head=None, rpn_pre_nms_top_n_train=2000, rpn_pre_nms_top_n_test=1000,
                 rpn_post_nms_top_n_train=2000, rpn_post_nms_top_n_test=1000, rpn_nms_thresh=0.7, rpn_fg_iou_thresh=0.7,
                 rpn_bg_iou_thresh=0.3, rpn_batch_size_per_image=256, rpn_positive_fraction=0.5, rpn_score_thresh=0.0,
                 box_roi_pool=None, box_head=None, box_predictor=None, box_score_thresh=0.05, box_nms_thresh=0.5,
                 box_detections_per_img=100, box_fg_iou_thresh=0.5, box_bg_iou_thresh=0.5, box_batch_size_per_image=512,
                 box_positive_fraction=0.25, bbox_reg_weights=None, **kwargs):
        super().__init__()
        if not hasattr(backbone, 'out_channels'):
            raise ValueError('backbone should contain an attribute out_channels specifying the number of output channels')
        if (num_classes is None) == (box_predictor is None):
            raise ValueError('exactly one of num_classes and box_predictor should be given')
        out_channels = backbone.out_channels
        if rpn_anchor_generator is None:
            rpn_anchor_generator = AnchorGenerator(((32,), (64,), (128,), (256,), (512,)), ((0.5, 1.0, 2.0),) * 5)
        if rpn_head is None:
            rpn_head = RPNHead(out_channels, rpn_anchor_generator.num_anchors_per_location()[0])
        self.rpn = RegionProposalNetwork(rpn_anchor_generator, rpn_head, rpn_fg_iou_thresh, rpn_bg_iou_thresh, rpn_batch_size_per_image,
                                         rpn_positive_fraction, dict(training=rpn_pre_nms_top_n_train, testing=rpn_pre_nms_top_n_test),
                                         dict(training=rpn_post_nms_top_n_train, testing=rpn_post_nms_top_n_test), rpn_nms_thresh,
                                         score_thresh=rpn_score_thresh)
        if box_roi_pool is None:
            box_roi_pool = MultiScaleRoIAlign(featmap_names=['0', '1', '2', '3'], output_size=7, sampling_ratio=2)
        if box_head is None:
            box_head = TwoMLPHead(out_channels * box_roi_pool.output_size[0] ** 2, 1024)
        if box_predictor is None:
            box_predictor = FastRCNNPredictor(1024, num_classes)
        self.roi_heads = RoIHeads(box_roi_pool, box_head, box_predictor, box_fg_iou_thresh, box_bg_iou_thresh, box_batch_size_per_image,
                                  box_positive_fraction, bbox_reg_weights, box_score_thresh, box_nms_thresh, box_detections_per_img)
        self.backbone = backbone
        self.transform = GeneralizedRCNNTransform(min_size, max_size, image_mean or [0.485, 0.456, 0.406],
                                                  image_std or [0.229, 0.224, 0.225], **kwargs)

    def forward(self, images, targets=None):
        if self.training and targets is None:
            raise ValueError('targets should not be None in training mode')
        original_image_sizes = original_sizes(images)
        images, targets = self.transform(images, targets)
        features = self.backbone(images.tensors)
        if isinstance(features, torch.Tensor):
            features = OrderedDict([('0', features)])
        proposals, proposal_losses = self.rpn(images, features, targets)
        detections, detector_losses = self.roi_heads(features, proposals, images.image_sizes, targets)
        if self.training:      # the four-key loss dict, in torchvision's order
            losses = dict(detector_losses)
            losses.update(proposal_losses)
            return losses
        return self.transform.postprocess(detections, images.image_sizes, original_image_sizes)
