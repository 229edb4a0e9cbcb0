"""Independent reference of sc2_rpn_proposals (include/sc2_bottleneck.h; torchvision's `RegionProposalNetwork.filter_proposals` with
the decode in front of it), written from the definition and not imported from the package -- plus the input generator the CPU and
GPU tests share.

* `select_ref`: the k greatest logits of one level, an exact integer result: NaN above every number, -0 equal to +0, ties by the
  lower index.
* `stage_a_ref`: scores and clipped boxes of GIVEN selected indices in float64 from the f32 inputs.
* `stage_b_ref`: the filters, the order (score descending, level ascending, rank ascending), greedy NMS within each level and the
  first P, sequentially in numpy float32 from a GIVEN candidate table: the comparisons and the IoU (`ref_detection.nms_ref`'s, every
  operation rounded once) are those of the kernel bit for bit, so that its result is the kernel's exactly when both start from the
  same table.
"""
import numpy as np

import ref_detection as RD

F32 = np.float32


def level_logits(objectness):
    """the head's objectness map [N,A,H,W] -> [N, n_l] in the level's index order t = (h W + w) A + a"""
    o = np.asarray(objectness)
    return o.transpose(0, 2, 3, 1).reshape(o.shape[0], -1)


def level_deltas(deltas):
    """the head's delta map [N,4A,H,W] (channel 4 a + c) -> [N, n_l, 4] in the same order"""
    d = np.asarray(deltas)
    N, A4, H, W = d.shape
    return d.reshape(N, A4 // 4, 4, H, W).transpose(0, 3, 4, 1, 2).reshape(N, -1, 4)


def select_ref(logits, K):
    """logits f32 [n] of one level of one image -> int64 [min(K, n)]: the indices of the greatest logits, in order -- NaN first (all
    NaNs equal), then descending value with -0 equal to +0; equal logits by ascending index.  The place in this list is the RANK."""
    v = np.asarray(logits, dtype=np.float64).reshape(-1)
    nan = np.isnan(v)
    order = np.lexsort((np.arange(v.shape[0]), -np.where(nan, 0.0, v), ~nan))      # (the LAST key is the primary one)
    return order[:min(int(K), v.shape[0])].astype(np.int64)


def select_batch(objectness_levels, K):
    """-> (index int32 [N,L,K], -1 behind k_l; k int32 [N,L]): `select_ref` of every (image, level)"""
    N, L = np.asarray(objectness_levels[0]).shape[0], len(objectness_levels)
    index, k = np.full((N, L, K), -1, dtype=np.int32), np.zeros((N, L), dtype=np.int32)
    for l, o in enumerate(objectness_levels):
        flat = level_logits(o)
        for i in range(N):
            s = select_ref(flat[i], K)
            index[i, l, :s.shape[0]] = s
            k[i, l] = s.shape[0]
    return index, k


def stage_a_ref(objectness_levels, delta_levels, anchors, image_sizes, index, k, weights, bbox_xform_clip):
    """The head's maps (f32 [N,A_l,H_l,W_l] / [N,4 A_l,H_l,W_l]), anchors f32 [T,4] of one image, image_sizes (h, w) per image, the
    selected level-local indices index [N,L,K] with k [N,L] of them per (image, level)
    -> (scores float64 [N,L,K], boxes float64 [N,L,K,4]), zeros behind k: score = 1 / (1 + exp(-logit)), the box
    BoxCoder.decode_single of (anchor, deltas) followed by the clip to the image.  The weights and the clip value are taken as the f32
    numbers the kernel receives."""
    N, L, K = index.shape
    scores, boxes = np.zeros((N, L, K)), np.zeros((N, L, K, 4))
    wx, wy, ww, wh = [float(F32(w)) for w in weights]
    clip = float(F32(bbox_xform_clip))
    anchors = np.asarray(anchors, dtype=np.float64)
    off = 0
    for l in range(L):
        lg, dl = level_logits(objectness_levels[l]).astype(np.float64), level_deltas(delta_levels[l]).astype(np.float64)
        for i in range(N):
            t = index[i, l, :k[i, l]].astype(np.int64)
            h, w = image_sizes[i]
            p, d = anchors[off + t], dl[i, t]
            with np.errstate(invalid='ignore', over='ignore'):
                scores[i, l, :t.shape[0]] = 1.0 / (1.0 + np.exp(-lg[i, t]))
                widths, heights = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]
                ctr_x, ctr_y = p[:, 0] + 0.5 * widths, p[:, 1] + 0.5 * heights
                dx, dy = d[:, 0] / wx, d[:, 1] / wy
                dw, dh = np.minimum(d[:, 2] / ww, clip), np.minimum(d[:, 3] / wh, clip)      # (np.minimum keeps a NaN)
                pcx, pcy = dx * widths + ctr_x, dy * heights + ctr_y
                half_w, half_h = 0.5 * (np.exp(dw) * widths), 0.5 * (np.exp(dh) * heights)
                b = np.stack([pcx - half_w, pcy - half_h, pcx + half_w, pcy + half_h], axis=1)
                b[:, 0::2] = np.minimum(np.maximum(b[:, 0::2], 0.0), float(w))
                b[:, 1::2] = np.minimum(np.maximum(b[:, 1::2], 0.0), float(h))
            boxes[i, l, :t.shape[0]] = b
        off += lg.shape[1]
    return scores, boxes


def survivors(cand_scores, cand_boxes, score_thresh, min_size):
    """bool [...] in f32: both sides >= min_size and score >= score_thresh, all inclusive (a NaN compares false)"""
    s, b = np.asarray(cand_scores, dtype=F32), np.asarray(cand_boxes, dtype=F32)
    with np.errstate(invalid='ignore'):
        return (s >= F32(score_thresh)) & ((b[..., 2] - b[..., 0]) >= F32(min_size)) & ((b[..., 3] - b[..., 1]) >= F32(min_size))


def _ordered(scores, boxes, k, score_thresh, min_size):
    """one image's table [L,K] -> (level, rank) of its survivors in key order: score descending, level ascending, rank ascending"""
    L, K = scores.shape
    alive = survivors(scores, boxes, score_thresh, min_size) & (np.arange(K)[None, :] < np.asarray(k)[:, None])
    lvl, rank = np.nonzero(alive)                                                 # ascending (level, rank)
    order = np.argsort(-scores[lvl, rank].astype(np.float64), kind='stable')      # descending score, ties as they stand
    return lvl[order], rank[order]


def stage_b_ref(cand_scores, cand_boxes, k, score_thresh, min_size, nms_thresh, P):
    """cand_scores f32 [N,L,K], cand_boxes f32 [N,L,K,4], k [N,L] -> per image (boxes f32 [m,4], scores f32 [m], levels int64 [m],
    ranks int64 [m]), m <= P: the survivors in key order, box j kept iff no earlier kept box of its LEVEL has IoU > nms_thresh with
    it, the first P kept."""
    s, b = np.asarray(cand_scores, dtype=F32), np.asarray(cand_boxes, dtype=F32)
    out = []
    for i in range(s.shape[0]):
        lvl, rank = _ordered(s[i], b[i], k[i], score_thresh, min_size)
        keep = RD.nms_ref(b[i][lvl, rank], lvl, nms_thresh) if lvl.shape[0] else np.zeros(0, dtype=bool)
        lvl, rank = lvl[keep][:P], rank[keep][:P]
        out.append((b[i][lvl, rank].copy(), s[i][lvl, rank].copy(), lvl.astype(np.int64), rank.astype(np.int64)))
    return out


def margins(cand_scores, cand_boxes, k, score_thresh, min_size, nms_thresh):
    """How far the decisions of stage B lie from flipping, in float64 on the given table: `score` = min |score - score_thresh| over
    the candidates with admissible sides, `side` = min |side - min_size| over all candidates, `iou` = min |IoU - nms_thresh| over
    the pairs the walk decides (an earlier KEPT box against a later survivor of its level), `gap` = the least difference of two
    adjacent DISTINCT scores in an image's ordered survivor list."""
    s, b = np.asarray(cand_scores, dtype=np.float64), np.asarray(cand_boxes, dtype=np.float64)
    N, L, K = s.shape
    live = np.arange(K)[None, None, :] < np.asarray(k)[:, :, None]
    with np.errstate(invalid='ignore'):
        sides = np.minimum(b[..., 2] - b[..., 0], b[..., 3] - b[..., 1])
        ok = np.isfinite(s) & np.isfinite(sides) & live
        score_m = np.abs(s - score_thresh)[ok & (sides >= min_size)]
        side_m = np.abs(sides - min_size)[ok]
    out = {'score': score_m.min() if score_m.size else np.inf, 'side': side_m.min() if side_m.size else np.inf, 'iou': np.inf,
           'gap': np.inf}
    for i in range(N):
        lvl, rank = _ordered(np.asarray(cand_scores[i], dtype=F32), np.asarray(cand_boxes[i], dtype=F32), k[i], score_thresh, min_size)
        steps = -np.diff(s[i][lvl, rank])
        if (steps > 0).any():
            out['gap'] = min(out['gap'], steps[steps > 0].min())
        for l in np.unique(lvl):
            bb = b[i][lvl[lvl == l], rank[lvl == l]]
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
def grid_anchors(level_shapes, image_size, seed=0):
    """anchors f32 [T,4] of one image in the order t = (h W + w) A + a per level: A boxes of a level-dependent size (and a few
    pixels of seeded jitter in their shapes) around every cell centre of an H x W grid laid over the image -- neighbours overlap
    heavily, as an RPN's do"""
    rng = np.random.RandomState(seed)
    ih, iw = image_size
    out = []
    for l, (A, H, W) in enumerate(level_shapes):
        sy, sx = ih / float(H), iw / float(W)
        cy, cx = (np.arange(H) + 0.5) * sy, (np.arange(W) + 0.5) * sx
        side = max(sy, sx) * 2.5
        shapes = side * (0.7 + 0.6 * rng.rand(A, 2))
        c = np.stack(np.broadcast_arrays(cx[None, :, None], cy[:, None, None]), axis=-1)      # [H,W,1,2] (x, y)
        c = np.broadcast_to(c, (H, W, A, 2))
        out.append(np.concatenate([c - shapes / 2, c + shapes / 2], axis=-1).reshape(-1, 4))
    return np.concatenate(out).round().astype(F32)


def random_case(level_shapes, N, image_size, seed, logit_scale=2.0, delta_scale=0.3, distinct=False):
    """Seeded head outputs of one batch: level_shapes = [(A_l, H_l, W_l)] -> (objectness levels f32 [N,A,H,W], delta levels
    f32 [N,4A,H,W], anchors f32 [T,4]).  distinct: every image's logits are a permutation of DISTINCT, evenly spaced values (no tie
    anywhere: what a comparison with an implementation that leaves ties unspecified needs)."""
    rng = np.random.RandomState(seed)
    T = sum(a * h * w for a, h, w in level_shapes)
    if distinct:
        flat = np.stack([(rng.permutation(T) - T / 2.0) * (2.0 * logit_scale / T) for _ in range(N)]).astype(F32)
    else:
        flat = (rng.randn(N, T) * logit_scale).astype(F32)
    obj, dl, off = [], [], 0
    for A, H, W in level_shapes:
        n = A * H * W
        obj.append(np.ascontiguousarray(flat[:, off:off + n].reshape(N, H, W, A).transpose(0, 3, 1, 2)))
        dl.append((rng.randn(N, 4 * A, H, W) * delta_scale).astype(F32))
        off += n
    return obj, dl, grid_anchors(level_shapes, image_size, seed)
