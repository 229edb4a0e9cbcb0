"""COCOeval's `bbox` protocol with its default parameters as a plain sequential float64 loop: the yardstick of the COCO box-AP
tests (include/sc2_bottleneck.h states the same definition).  Written from the published protocol; it shares no code with
sc2bench_amd/coco_eval.py.  Python floats are IEEE f64 and every operation below is rounded once.

    evaluate(gt_dict, predictions) -> {'precision' [10,101,K,4,3], 'recall' [10,K,4,3], 'stats' [12], 'lines' [12 str]}
    predictions: {image id: {'boxes' [n,4] xyxy f32, 'scores' [n], 'labels' [n]}} (numpy arrays, lists or tensors); every key is an
    evaluated image, also one with no boxes.
"""
import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RNG = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))
AREA_NAMES = ('all', 'small', 'medium', 'large')
EPS = float(np.spacing(1))


def to_xywh(box):
    """(x1,y1,x2,y2) in f32 -> [x1, y1, f32(x2-x1), f32(y2-y1)] as Python floats"""
    x1, y1, x2, y2 = (np.float32(v) for v in box)
    return [float(x1), float(y1), float(np.float32(x2 - x1)), float(np.float32(y2 - y1))]


def iou(d, g, crowd):
    w = min(d[0] + d[2], g[0] + g[2]) - max(d[0], g[0])
    h = min(d[1] + d[3], g[1] + g[3]) - max(d[1], g[1])
    if w <= 0 or h <= 0:
        return 0.0
    i = w * h
    u = d[2] * d[3] if crowd else d[2] * d[3] + g[2] * g[3] - i
    return float(np.float64(i) / np.float64(u))


def match_segment(dets, gts, gt_area, gt_crowd):
    """One (image, category): dets [[x,y,w,h]] ALREADY in processing order, gts [[x,y,w,h]] in annotation order.
    -> (matched[a][t][d], ignored[a][t][d] as 0/1 lists, npig[a], which[a][t][d]: the matched ground truth's index or None)."""
    D, G = len(dets), len(gts)
    ious = [[iou(d, g, bool(c)) for g, c in zip(gts, gt_crowd)] for d in dets]
    matched = [[[0] * D for _ in IOU_THRS] for _ in AREA_RNG]
    ignored = [[[0] * D for _ in IOU_THRS] for _ in AREA_RNG]
    which = [[[None] * D for _ in IOU_THRS] for _ in AREA_RNG]
    npig = []
    for a, (lo, hi) in enumerate(AREA_RNG):
        g_ign = [1 if (gt_crowd[g] or gt_area[g] < lo or gt_area[g] > hi) else 0 for g in range(G)]
        order = [g for g in range(G) if not g_ign[g]] + [g for g in range(G) if g_ign[g]]      # non-ignored first, stable
        npig.append(sum(1 for g in range(G) if not g_ign[g]))
        for ti, t in enumerate(IOU_THRS):
            taken = [False] * G
            for di in range(D):
                best = min(float(t), 1 - 1e-10)
                m = None
                for g in order:
                    if taken[g] and not gt_crowd[g]:
                        continue
                    if m is not None and not g_ign[m] and g_ign[g]:
                        break
                    if ious[di][g] < best:
                        continue
                    best = ious[di][g]
                    m = g
                if m is not None:
                    matched[a][ti][di] = 1
                    ignored[a][ti][di] = g_ign[m]
                    taken[m] = True
                    which[a][ti][di] = m
                else:
                    area = dets[di][2] * dets[di][3]
                    ignored[a][ti][di] = 1 if (area < lo or area > hi) else 0
    return matched, ignored, npig, which


def flag_words(matched, ignored, d):
    """the int32 words sc2_coco_match writes for detection d: per area range, bit t matched, bit 10+t ignored"""
    return [sum(matched[a][t][d] << t for t in range(10)) | (sum(ignored[a][t][d] << t for t in range(10)) << 10) for a in range(4)]


def curves(entries, npig):
    """entries: [(matched[t], ignored[t])] of one (category, area range, maxDet) ALREADY in score order; -> (precision [10][101],
    recall [10]), or None where npig == 0."""
    if npig == 0:
        return None
    precision, recall = [], []
    for t in range(len(IOU_THRS)):
        tp = fp = 0
        rc, pr = [], []
        for mt, ig in entries:
            if not ig[t]:
                if mt[t]:
                    tp += 1
                else:
                    fp += 1
            rc.append(float(np.float64(tp) / np.float64(npig)))
            pr.append(float(np.float64(tp) / (np.float64(fp) + np.float64(tp) + np.float64(EPS))))
        for i in range(len(pr) - 1, 0, -1):
            if pr[i] > pr[i - 1]:
                pr[i - 1] = pr[i]
        row, at = [], 0
        for r in REC_THRS:      # (rc never decreases and recThrs ascends: the first entry reaching r lies at or behind the last one's)
            while at < len(rc) and rc[at] < r:
                at += 1
            row.append(pr[at] if at < len(rc) else 0.0)
        precision.append(row)
        recall.append(rc[-1] if rc else 0.0)
    return precision, recall


def segments(gt, predictions):
    """-> (cat_ids, img_ids, {(image id, category id): (dets xywh in processing order, scores, gts xywh, gt_area, gt_crowd)})"""
    cat_ids = sorted(int(c['id']) for c in gt['categories'])
    img_ids = sorted(int(i) for i in predictions)
    out = {}
    for image_id in img_ids:
        for c in cat_ids:
            out[(image_id, c)] = ([], [], [], [], [])
    for ann in gt['annotations']:
        key = (int(ann['image_id']), int(ann['category_id']))
        if key in out:
            out[key][2].append([float(v) for v in ann['bbox']])
            out[key][3].append(float(ann['area']))
            out[key][4].append(1 if ann.get('iscrowd', 0) else 0)
    for image_id, pred in predictions.items():
        if pred is None or len(pred) == 0:
            continue
        boxes = np.asarray(pred['boxes'], dtype=np.float32).reshape(-1, 4)
        scores = np.asarray(pred['scores'], dtype=np.float32).reshape(-1)
        labels = np.asarray(pred['labels']).reshape(-1)
        per_cat = {}
        for i in range(len(scores)):
            per_cat.setdefault(int(labels[i]), []).append(i)
        for c, idx in per_cat.items():
            if (int(image_id), c) not in out:
                continue      # a label outside the categories
            idx = sorted(idx, key=lambda i: -float(scores[i]))[:MAX_DETS[-1]]      # stable: ties keep their position
            seg = out[(int(image_id), c)]
            seg[0].extend(to_xywh(boxes[i]) for i in idx)
            seg[1].extend(float(scores[i]) for i in idx)
    return cat_ids, img_ids, out


def summarize(precision, recall):
    """-> (stats [12], the twelve printed lines)"""
    def stat(ap, iou_thr, area, max_det):
        a, m = AREA_NAMES.index(area), MAX_DETS.index(max_det)
        s = precision if ap else recall
        if iou_thr is not None:
            s = s[np.where(iou_thr == IOU_THRS)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        s = s[s > -1]
        return -1.0 if s.size == 0 else float(np.mean(s))
    specs = [(1, None, 'all', 100), (1, .5, 'all', 100), (1, .75, 'all', 100), (1, None, 'small', 100), (1, None, 'medium', 100),
             (1, None, 'large', 100), (0, None, 'all', 1), (0, None, 'all', 10), (0, None, 'all', 100), (0, None, 'small', 100),
             (0, None, 'medium', 100), (0, None, 'large', 100)]
    stats = np.array([stat(*s) for s in specs])
    lines = []
    for (ap, iou_thr, area, max_det), v in zip(specs, stats):
        rng = '0.50:0.95' if iou_thr is None else '{:0.2f}'.format(iou_thr)
        lines.append(' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(
            'Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', rng, area, max_det, v))
    return stats, lines


def evaluate(gt, predictions):
    cat_ids, img_ids, segs = segments(gt, predictions)
    K = len(cat_ids)
    precision = -np.ones((10, 101, K, 4, 3))
    recall = -np.ones((10, K, 4, 3))
    results = {key: match_segment(s[0], s[2], s[3], s[4]) for key, s in segs.items()}
    for k, c in enumerate(cat_ids):
        for a in range(4):
            npig = sum(results[(i, c)][2][a] for i in img_ids)
            for mi, max_det in enumerate(MAX_DETS):
                entries = []      # (score, matched[t], ignored[t]) of the first max_det detections of every image, ascending image id
                for i in img_ids:
                    matched, ignored = results[(i, c)][:2]
                    scores = segs[(i, c)][1]
                    for d in range(min(len(scores), max_det)):
                        entries.append((scores[d], [matched[a][t][d] for t in range(10)], [ignored[a][t][d] for t in range(10)]))
                entries.sort(key=lambda e: -e[0])      # stable
                got = curves([(e[1], e[2]) for e in entries], npig)
                if got is not None:
                    precision[:, :, k, a, mi] = np.array(got[0])
                    recall[:, k, a, mi] = np.array(got[1])
    stats, lines = summarize(precision, recall)
    return {'precision': precision, 'recall': recall, 'stats': stats, 'lines': lines, 'segments': segs, 'matches': results,
            'cat_ids': cat_ids, 'img_ids': img_ids}
