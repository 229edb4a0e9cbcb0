"""Independent reference of sc2_det_postprocess (include/sc2_bottleneck.h; torchvision's `RoIHeads.postprocess_detections`), written
from the definition and not imported from the package -- plus the input generator the CPU and GPU tests share.

* `stage_a_ref`: scores and clipped boxes of every (proposal, foreground class) in float64 from the f32 inputs.
* `stage_b_ref`: the filters, the stable descending order, greedy NMS within each class and the first D, sequentially in numpy
  float32 from a GIVEN candidate table: the comparisons and the IoU (`ref_detection.nms_ref`'s, every operation rounded once) are
  those of the kernel bit for bit, so that its result is the kernel's exactly when both start from the same table.
"""
import numpy as np

import ref_detection as RD

F32 = np.float32


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))])


def stage_a_ref(logits, deltas, proposals, counts, image_sizes, weights, bbox_xform_clip):
    """logits f32 [R,C], deltas f32 [R,4C], proposals f32 [R,4], counts: proposals per image, image_sizes: (h, w) per image
    -> (scores float64 [R,C-1], boxes float64 [R,C-1,4]): softmax over the C logits without the background column, and
    BoxCoder.decode_single followed by the clip to the image.  The weights and the clip value are taken as the f32 numbers the
    kernel receives.  A row with a NaN or +infinite logit comes out all NaN, as softmax makes it."""
    lg = np.asarray(logits, dtype=np.float64)
    R, C = lg.shape
    d = np.asarray(deltas, dtype=np.float64).reshape(R, C, 4)
    p = np.asarray(proposals, dtype=np.float64)
    wx, wy, ww, wh = [float(F32(w)) for w in weights]
    clip = float(F32(bbox_xform_clip))
    with np.errstate(invalid='ignore', over='ignore'):
        e = np.exp(lg - lg.max(axis=1, keepdims=True)) if R else np.zeros((0, C))
        scores = e / e.sum(axis=1, keepdims=True)
        widths, heights = (p[:, 2] - p[:, 0])[:, None], (p[:, 3] - p[:, 1])[:, None]
        ctr_x, ctr_y = p[:, 0:1] + 0.5 * widths, p[:, 1:2] + 0.5 * heights
        dx, dy = d[:, :, 0] / wx, d[:, :, 1] / wy
        dw, dh = np.minimum(d[:, :, 2] / ww, clip), np.minimum(d[:, :, 3] / wh, clip)      # (np.minimum keeps a NaN)
        pcx, pcy = dx * widths + ctr_x, dy * heights + ctr_y
        half_w, half_h = 0.5 * (np.exp(dw) * widths), 0.5 * (np.exp(dh) * heights)
        boxes = np.stack([pcx - half_w, pcy - half_h, pcx + half_w, pcy + half_h], axis=2)
        off = _offsets(counts)
        for i, (h, w) in enumerate(image_sizes):
            b = boxes[off[i]:off[i + 1]]
            b[:, :, 0::2] = np.minimum(np.maximum(b[:, :, 0::2], 0.0), float(w))
            b[:, :, 1::2] = np.minimum(np.maximum(b[:, :, 1::2], 0.0), float(h))
    return scores[:, 1:], boxes[:, 1:]


def survivors(cand_scores, cand_boxes, score_thresh, min_size):
    """bool [R,C-1] in f32: score > score_thresh and both sides >= min_size (a NaN compares false)"""
    s, b = np.asarray(cand_scores, dtype=F32), np.asarray(cand_boxes, dtype=F32)
    with np.errstate(invalid='ignore'):
        return (s > F32(score_thresh)) & ((b[..., 2] - b[..., 0]) >= F32(min_size)) & ((b[..., 3] - b[..., 1]) >= F32(min_size))


def stage_b_ref(cand_scores, cand_boxes, counts, score_thresh, min_size, nms_thresh, D):
    """cand_scores f32 [R,C-1], cand_boxes f32 [R,C-1,4] -> per image (boxes f32 [k,4], scores f32 [k], labels int64 [k]), k <= D.
    Per image: the survivors in the order of a STABLE descending sort by score over the flat index r_local * (C-1) + (c-1); box j is
    kept iff no earlier kept box of its class has IoU > nms_thresh with it; the first D kept.  Boxes of different classes never
    meet, so the walk runs class by class over the ordered list (what one walk with groups gives, without its n^2 / 2 pair tests)."""
    s, b = np.asarray(cand_scores, dtype=F32), np.asarray(cand_boxes, dtype=F32)
    nc = s.shape[1]
    alive = survivors(s, b, score_thresh, min_size)
    off = _offsets(counts)
    out = []
    for i in range(len(counts)):
        si, bi = s[off[i]:off[i + 1]].reshape(-1), b[off[i]:off[i + 1]].reshape(-1, 4)
        flat = np.nonzero(alive[off[i]:off[i + 1]].reshape(-1))[0]                 # ascending flat index
        flat = flat[np.argsort(-si[flat].astype(np.float64), kind='stable')]       # descending score, ties by flat index
        cls = flat % nc
        keep = np.zeros(flat.shape[0], dtype=bool)
        for c in np.unique(cls):
            sel = np.nonzero(cls == c)[0]
            keep[sel] = RD.nms_ref(bi[flat[sel]], np.zeros(sel.shape[0], dtype=np.int64), nms_thresh)
        flat = flat[keep][:D]
        out.append((bi[flat].copy(), si[flat].copy(), (flat % nc + 1).astype(np.int64)))
    return out


def margins(cand_scores, cand_boxes, counts, score_thresh, min_size, nms_thresh):
    """How far the decisions of stage B lie from flipping, in float64 on the given table: (score, side, iou) =
    min |score - score_thresh| over all candidates with admissible sides, min | side - min_size | over all candidates, and
    min |IoU - nms_thresh| over the pairs the walk decides (an earlier KEPT box against a later survivor of its class), plus
    `gap`: the least difference of two adjacent DISTINCT scores in an image's ordered survivor list."""
    s, b = np.asarray(cand_scores, dtype=np.float64), np.asarray(cand_boxes, dtype=np.float64)
    nc = s.shape[1]
    alive = survivors(cand_scores, cand_boxes, score_thresh, min_size)
    with np.errstate(invalid='ignore'):
        sides = np.minimum(b[..., 2] - b[..., 0], b[..., 3] - b[..., 1])
        ok = np.isfinite(s) & np.isfinite(sides)
        score_m = np.abs(s - score_thresh)[ok & (sides >= min_size)]
        side_m = np.abs(sides - min_size)[ok]
    out = {'score': score_m.min() if score_m.size else np.inf, 'side': side_m.min() if side_m.size else np.inf, 'iou': np.inf,
           'gap': np.inf}
    off = _offsets(counts)
    for i in range(len(counts)):
        si, bi = s[off[i]:off[i + 1]].reshape(-1), b[off[i]:off[i + 1]].reshape(-1, 4)
        flat = np.nonzero(alive[off[i]:off[i + 1]].reshape(-1))[0]
        flat = flat[np.argsort(-si[flat], kind='stable')]
        steps = -np.diff(si[flat])
        if (steps > 0).any():
            out['gap'] = min(out['gap'], steps[steps > 0].min())
        cls = flat % nc
        for c in np.unique(cls):
            bb = bi[flat[cls == c]]
            keep = RD.nms_ref(bb.astype(F32), np.zeros(bb.shape[0], dtype=np.int64), nms_thresh)
            area = (bb[:, 2] - bb[:, 0]) * (bb[:, 3] - bb[:, 1])
            for j in np.nonzero(keep)[0]:
                later = slice(j + 1, None)
                w = np.maximum(0, np.minimum(bb[j, 2], bb[later, 2]) - np.maximum(bb[j, 0], bb[later, 0]))
                h = np.maximum(0, np.minimum(bb[j, 3], bb[later, 3]) - np.maximum(bb[j, 1], bb[later, 1]))
                with np.errstate(invalid='ignore', divide='ignore'):
                    dist = np.abs(w * h / (area[j] + area[later] - w * h) - nms_thresh)
                dist = dist[np.isfinite(dist)]
                if dist.size:
                    out['iou'] = min(out['iou'], dist.min())
    return out


# ------------------------------------------------------------------------------------------------ shared inputs
def random_case(counts, C, image_sizes, seed, logit_scale=4.0, delta_scale=1.0, clusters=6):
    """Seeded inputs of one batch: proposals clustered so that boxes of a class overlap heavily, logits spread by `logit_scale` (a
    larger value: fewer classes of a row above the score threshold), deltas of a few tenths of a box.
    -> logits f32 [R,C], deltas f32 [R,4C], proposals f32 [R,4]"""
    rng = np.random.RandomState(seed)
    R = int(sum(counts))
    props = np.zeros((R, 4), dtype=F32)
    r = 0
    for k, (h, w) in zip(counts, image_sizes):
        centres = rng.rand(clusters, 2) * [w, h]
        c = centres[rng.randint(0, clusters, k)] + rng.randn(k, 2) * 6.0
        wh = 12.0 + rng.rand(k, 2) * 60.0
        props[r:r + k] = np.concatenate([c - wh / 2, c + wh / 2], axis=1)
        r += k
    logits = (rng.randn(R, C) * logit_scale).astype(F32)
    deltas = (rng.randn(R, 4 * C) * delta_scale).astype(F32)
    return logits, deltas, props
