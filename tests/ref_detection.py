"""Independent reference of the two detection kernels (include/sc2_bottleneck.h: sc2_nms, sc2_roi_align), written from the
definitions and not imported from the package -- plus the input generators the CPU and GPU tests share.

* `nms_ref`: a sequential loop in numpy float32, every operation rounded once and in the order the header states, so that
  its decisions are the kernel's bit for bit.
* `roi_align_ref`: float64, straight from the definition (torchvision's aligned=False RoIAlign).
"""
import numpy as np

F32 = np.float32


def nms_ref(boxes, groups, thr):
    """boxes f32 [n,4] ALREADY in processing order, groups [n] -> bool keep [n].  Box i is kept iff no earlier kept box of
    its group has IoU > thr (strictly)."""
    b = np.ascontiguousarray(boxes, dtype=F32)
    g = np.asarray(groups)
    n = b.shape[0]
    thr = F32(thr)
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    area = (x2 - x1) * (y2 - y1)                      # f32, one rounding per operation
    keep = np.zeros(n, dtype=bool)
    suppressed = np.zeros(n, dtype=bool)
    with np.errstate(invalid='ignore', divide='ignore'):
        for i in range(n):                            # the sequential walk; the inner comparison runs over the later boxes
            if suppressed[i]:
                continue
            keep[i] = True
            w = np.maximum(F32(0), np.minimum(x2[i], x2[i + 1:]) - np.maximum(x1[i], x1[i + 1:]))
            h = np.maximum(F32(0), np.minimum(y2[i], y2[i + 1:]) - np.maximum(y1[i], y1[i + 1:]))
            inter = w * h
            iou = inter / (area[i] + area[i + 1:] - inter)
            assert iou.dtype == F32
            suppressed[i + 1:] |= (iou > thr) & (g[i + 1:] == g[i])
    return keep


def batched_nms_ref(boxes, scores, idxs, thr):
    """-> kept original indices in processing order (stable descending score sort: ties keep the lower index first)"""
    order = np.argsort(-np.asarray(scores, dtype=np.float64), kind='stable')
    keep = nms_ref(np.asarray(boxes, dtype=F32)[order], np.asarray(idxs)[order], thr)
    return order[keep]


def _bilinear(fm, y, x):
    """fm float64 [C,H,W]; one sample of torchvision's bilinear_interpolate -> [C]"""
    C, H, W = fm.shape
    if y < -1.0 or y > H or x < -1.0 or x > W:
        return np.zeros(C)
    y, x = max(y, 0.0), max(x, 0.0)
    yl, xl = int(y), int(x)
    if yl >= H - 1:
        yh = yl = H - 1
        y = float(yl)
    else:
        yh = yl + 1
    if xl >= W - 1:
        xh = xl = W - 1
        x = float(xl)
    else:
        xh = xl + 1
    ly, lx = y - yl, x - xl
    hy, hx = 1.0 - ly, 1.0 - lx
    return hy * hx * fm[:, yl, xl] + hy * lx * fm[:, yl, xh] + ly * hx * fm[:, yh, xl] + ly * lx * fm[:, yh, xh]


def roi_samples(roi, scale, P, S):
    """float64 sample coordinates of one RoI (x1, y1, x2, y2): (ys [P*S], xs [P*S])"""
    out = []
    for lo, hi in ((roi[1], roi[3]), (roi[0], roi[2])):
        start, end = float(lo) * scale, float(hi) * scale
        bin_ = max(end - start, 1.0) / P
        out.append(np.array([start + p * bin_ + (i + 0.5) * bin_ / S for p in range(P) for i in range(S)]))
    return out[0], out[1]


def roi_align_ref(feats, scales, rois, levels, P, S):
    """feats: list of arrays [N,C,H,W] (any float dtype: evaluated in float64), rois [K,5], levels [K] -> float64 [K,C,P,P]"""
    feats = [np.asarray(f, dtype=np.float64) for f in feats]
    K, C = len(rois), feats[0].shape[1]
    out = np.zeros((K, C, P, P))
    for k in range(K):
        fm = feats[int(levels[k])][int(rois[k][0])]
        ys, xs = roi_samples(np.asarray(rois[k][1:], dtype=np.float64), float(scales[int(levels[k])]), P, S)
        for ph in range(P):
            for pw in range(P):
                acc = np.zeros(C)
                for iy in range(S):
                    for ix in range(S):
                        acc += _bilinear(fm, ys[ph * S + iy], xs[pw * S + ix])
                out[k, :, ph, pw] = acc / (S * S)
    return out


# ------------------------------------------------------------------------------------------------ shared inputs
def random_boxes(n, n_groups, seed, extent=200.0):
    """n boxes with heavy overlap (clustered centres), f32, plus descending-ish scores with ties and group labels"""
    rng = np.random.RandomState(seed)
    centres = rng.rand(max(1, n // 6), 2) * extent
    c = centres[rng.randint(0, len(centres), n)] + rng.randn(n, 2) * 4.0
    wh = 8.0 + rng.rand(n, 2) * 40.0
    boxes = np.concatenate([c - wh / 2, c + wh / 2], axis=1).astype(F32)
    scores = (rng.randint(0, max(2, n // 2), n) / float(max(2, n // 2))).astype(F32)      # many tied scores
    groups = rng.randint(0, n_groups, n).astype(np.int64)
    return boxes, scores, groups


def quarter_grid_boxes(n, seed):
    """boxes on the quarter-pixel grid drawn from a small set of shapes at a few offsets: every coordinate, area and
    intersection is exact in f32 and many pairs have IoU exactly 1/2 or 7/10 (e.g. [0,0,2,2] / [0,0,2,1]; 7 x 10 / 10 x 10)"""
    rng = np.random.RandomState(seed)
    shapes = np.array([[2, 2], [2, 1], [1, 2], [10, 10], [7, 10], [10, 7], [4, 4], [4, 2], [2.5, 2.5], [2.5, 1.25]])
    origin = rng.randint(0, 3, (n, 2)) * 0.25 * (rng.rand(n, 1) < 0.3)        # most boxes share the origin of their cluster
    cluster = rng.randint(0, 4, (n, 1)) * 64.0
    wh = shapes[rng.randint(0, len(shapes), n)]
    x1y1 = cluster + origin
    boxes = np.concatenate([x1y1, x1y1 + wh], axis=1).astype(F32)
    scores = (rng.randint(0, 50, n) / 50.0).astype(F32)
    return boxes, scores, np.zeros(n, dtype=np.int64)


IMAGE = (160, 208)                      # RoIAlign cases: image height x width; maps at strides 4, 8, 16
MAPS = ((40, 52), (20, 26), (10, 13))
SCALES = (0.25, 0.125, 0.0625)
EXCLUDE = 2.0 ** -10                    # RoIs with a sample this close to -1 or H / W (the definition's jumps) are dropped


def roi_features(C, seed, n_images=2):
    rng = np.random.RandomState(seed)
    return [rng.randn(n_images, C, h, w).astype(F32) for h, w in MAPS]


def roi_cases(K, seed, P, S, mode='mixed', n_images=2):
    """K RoIs [K,5] + levels [K]: inside the image, straddling each border, degenerate (x2 < x1) and wholly outside.
    mode 'mixed': spread over the three maps; 'one': all on map 1; 'skip': maps 0 and 2 only (map 1 has no RoI).
    RoIs with a float64 sample within EXCLUDE of a jump of the definition are dropped and redrawn as inside boxes;
    -> (rois f32, levels int64, number dropped)."""
    rng = np.random.RandomState(seed)
    Hh, Ww = IMAGE
    rois, levels, dropped = [], [], 0
    for k in range(K):
        kind = k % 8
        lvl = {'mixed': k % 3, 'one': 1, 'skip': (0, 2)[k % 2]}[mode]
        for attempt in range(2):
            if kind <= 2 or attempt:                      # inside
                x1, y1 = rng.rand() * (Ww - 40), rng.rand() * (Hh - 40)
                x2, y2 = x1 + 2 + rng.rand() * 38, y1 + 2 + rng.rand() * 38
            elif kind == 3:                               # left / top border
                x1, y1, x2, y2 = -rng.rand() * 30, -rng.rand() * 30, rng.rand() * 60, rng.rand() * 60
            elif kind == 4:                               # right / bottom border
                x1, y1, x2, y2 = Ww - rng.rand() * 60, Hh - rng.rand() * 60, Ww + rng.rand() * 40, Hh + rng.rand() * 40
            elif kind == 5:                               # degenerate
                x1, y1 = rng.rand() * Ww, rng.rand() * Hh
                x2, y2 = x1 - rng.rand() * 10, y1 - rng.rand() * 10
            elif kind == 6:                               # wholly outside, beyond -1 map pixel
                x1, y1, x2, y2 = -300 - rng.rand() * 50, -300 - rng.rand() * 50, -100 - rng.rand() * 50, -100 - rng.rand() * 50
            else:                                         # wholly outside on the far side
                x1, y1, x2, y2 = Ww + 40 + rng.rand() * 20, Hh + 40 + rng.rand() * 20, Ww + 100, Hh + 100
            roi = np.array([x1, y1, x2, y2], dtype=F32)
            ys, xs = roi_samples(roi.astype(np.float64), SCALES[lvl], P, S)
            h, w = MAPS[lvl]
            near = min(np.abs(ys + 1).min(), np.abs(ys - h).min(), np.abs(xs + 1).min(), np.abs(xs - w).min())
            if near >= EXCLUDE:
                break
            dropped += 1
        rois.append([float(rng.randint(0, n_images))] + roi.tolist())
        levels.append(lvl)
    return np.array(rois, dtype=F32), np.array(levels, dtype=np.int64), dropped


def chain_across_blocks():
    """130 far-apart boxes in processing order (descending scores); `chain_case` places the chain among them"""
    n = 130
    boxes = np.zeros((n, 4), dtype=F32)
    for i in range(n):
        boxes[i] = [100.0 * i, 0, 100.0 * i + 10, 10]
    return boxes, np.linspace(1.0, 0.0, n).astype(F32), np.zeros(n, dtype=np.int64)


def chain_case(thr):
    """the chain across the 64-block boundary: A at index 62, two copies of B at 63 and 64, C at 65, with A suppressing B, B
    overlapping C above the threshold and A not -> A and C stay, both B go"""
    boxes, scores, groups = chain_across_blocks()
    # height-10 boxes shifted along x by d: IoU(shift d) = (10 - d) / (10 + d); IoU(shift 2d) = (10 - 2d) / (10 + 2d)
    d = {0.5: 2.0, 0.7: 1.0}[thr]          # 0.5: 8/12 = 0.667 > 0.5, 6/14 = 0.43 < 0.5;  0.7: 9/11 = 0.82 > 0.7, 8/12 = 0.667 < 0.7
    x0 = 6200.0
    boxes[62] = [x0, 0, x0 + 10, 10]
    boxes[63] = boxes[64] = [x0 + d, 0, x0 + d + 10, 10]
    boxes[65] = [x0 + 2 * d, 0, x0 + 2 * d + 10, 10]
    return boxes, scores, groups


def nms_cases():
    """(name, boxes f32 [n,4], scores f32 [n], groups int64 [n], threshold) of every NMS case the CPU and GPU tests run"""
    cases = []
    for thr in (0.5, 0.7):
        for n in (1, 63, 64, 65, 129, 1000, 4097):
            for ng in (1, 5):
                cases.append(('random-n{}-g{}-t{}'.format(n, ng, thr),) + random_boxes(n, ng, seed=n * 7 + ng) + (thr,))
        same = np.tile(np.array([[3.0, 4.0, 30.0, 40.0]], dtype=F32), (200, 1))
        sc = np.linspace(1.0, 0.5, 200).astype(F32)
        cases.append(('identical-g1-t{}'.format(thr), same, sc, np.zeros(200, dtype=np.int64), thr))
        cases.append(('identical-g5-t{}'.format(thr), same, sc, (np.arange(200) % 5).astype(np.int64), thr))
        cases.append(('chain-t{}'.format(thr),) + chain_case(thr) + (thr,))
        b, _, g = random_boxes(129, 2, seed=99)
        cases.append(('tied-t{}'.format(thr), b, np.full(129, 0.25, dtype=F32), g, thr))
        for n in (129, 1000):
            cases.append(('quarter-n{}-t{}'.format(n, thr),) + quarter_grid_boxes(n, seed=n) + (thr,))
    return cases
