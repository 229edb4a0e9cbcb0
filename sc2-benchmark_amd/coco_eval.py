"""COCO box AP without pycocotools: `CocoBoxEvaluator` has the interface of the reference's `CocoEvaluator`
(script/task/coco/eval.py: update / synchronize_between_processes / accumulate / summarize / coco_eval['bbox'].stats) and computes
COCOeval's `bbox` protocol with its default parameters, stated in include/sc2_bottleneck.h and restated sequentially in
tests/ref_coco.py.

`update` only appends: a model's outputs stay where they are.  `accumulate` groups and sorts every buffered detection with a few
stable `torch.sort` calls on the tensors' device, then

  * device tensors (and `hip.host_policy.coco_eval_hip`): ONE `sc2_coco_match` launch over all (image, category) segments and ONE
    `sc2_coco_accumulate` launch over all (category, area range, maxDet) curves -- one copy to the host at the end;
  * CPU tensors, or the switch off: the numpy host path below, with the same results bit for bit.
"""
import json

import numpy as np
import torch

from . import hip
from .dataparallel import all_gather_picklable

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RNG = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)
AREA_LABELS = ('all', 'small', 'medium', 'large')
# (average precision?, IoU threshold or None for all, area range, maxDets) of the twelve statistics, in pycocotools' order
STAT_SPECS = ((True, None, 'all', 100), (True, .5, 'all', 100), (True, .75, 'all', 100), (True, None, 'small', 100),
              (True, None, 'medium', 100), (True, None, 'large', 100), (False, None, 'all', 1), (False, None, 'all', 10),
              (False, None, 'all', 100), (False, None, 'small', 100), (False, None, 'medium', 100), (False, None, 'large', 100))


def _gt_dict(gt):
    """A COCO dictionary, a path to its JSON, or anything with a `.dataset` attribute holding one (a pycocotools.COCO) -> the dictionary."""
    if isinstance(gt, str) or hasattr(gt, '__fspath__'):
        with open(gt) as f:
            gt = json.load(f)
    elif not isinstance(gt, dict) and isinstance(getattr(gt, 'dataset', None), dict):
        gt = gt.dataset
    if not isinstance(gt, dict) or 'annotations' not in gt or 'categories' not in gt:
        raise ValueError('ground truth must be a COCO dictionary (images, annotations, categories), a path to its JSON, or an object '
                         'whose .dataset is one; got {}'.format(type(gt).__name__))
    return gt


class BoxEval(object):
    """What `COCOeval` leaves behind for the reference's callers: `stats` (12 values), `eval` (precision [T,R,K,A,M], recall [T,K,A,M],
    counts) and the parameters."""

    def __init__(self, cat_ids):
        self.cat_ids = list(cat_ids)
        self.iou_thrs, self.rec_thrs, self.max_dets, self.area_rng = IOU_THRS, REC_THRS, MAX_DETS, AREA_RNG
        self.eval = {}
        self.stats = np.zeros(0)
        self.path = None         # 'hip' or 'host': what accumulate ran on

    def _stat(self, ap, iou_thr, area, max_det):
        a, m = AREA_LABELS.index(area), MAX_DETS.index(max_det)
        s = self.eval['precision'] if ap else self.eval['recall']
        if iou_thr is not None:
            s = s[np.where(iou_thr == self.iou_thrs)[0]]
        s = s[:, :, :, a, m] if ap else s[:, :, a, m]
        kept = s[s > -1]
        return -1.0 if kept.size == 0 else float(np.mean(kept))

    def summarize(self):
        if not self.eval:
            raise RuntimeError('Please run accumulate() first')
        self.stats = np.array([self._stat(*spec) for spec in STAT_SPECS], dtype=np.float64)
        for (ap, iou_thr, area, max_det), value in zip(STAT_SPECS, self.stats):
            iou = '{:0.2f}:{:0.2f}'.format(self.iou_thrs[0], self.iou_thrs[-1]) if iou_thr is None else '{:0.2f}'.format(iou_thr)
            print(' {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}'.format(
                'Average Precision' if ap else 'Average Recall', '(AP)' if ap else '(AR)', iou, area, max_det, value))
        return self.stats


class CocoBoxEvaluator(object):
    def __init__(self, gt, iou_types=('bbox',)):
        if isinstance(iou_types, str):
            iou_types = (iou_types,)
        missing = [t for t in iou_types if t != 'bbox']
        if missing:
            raise ValueError('CocoBoxEvaluator computes box AP only (iou type "bbox"): {} needs mask / keypoint evaluation, which this '
                             'package does not have (it builds faster_rcnn_model only)'.format(', '.join(repr(t) for t in missing)))
        self.iou_types = tuple(iou_types)
        gt = _gt_dict(gt)
        self.cat_ids = sorted(int(c['id']) for c in gt['categories'])
        cat_index = {c: k for k, c in enumerate(self.cat_ids)}
        self._gt = {}            # image id -> [(category index, x, y, w, h, area, iscrowd)] in annotation order
        for ann in gt['annotations']:
            k = cat_index.get(int(ann['category_id']))
            if k is None:
                continue
            x, y, w, h = (float(v) for v in ann['bbox'])
            self._gt.setdefault(int(ann['image_id']), []).append((k, x, y, w, h, float(ann['area']), int(bool(ann.get('iscrowd', 0)))))
        self.coco_eval = {t: BoxEval(self.cat_ids) for t in self.iou_types}
        self.img_ids = []
        self._preds = []         # (image id, boxes f32 [n,4], scores [n], labels [n]) as given
        self._seen = set()

    # ------------------------------------------------------------------------------------------------------------ buffering
    def update(self, predictions):
        """{image id: {'boxes' [n,4] xyxy, 'scores' [n], 'labels' [n]}}: appended as they are (no copy, no synchronisation).  An image
        with an empty (or no) prediction still counts: its ground truths are misses."""
        for image_id in sorted(predictions.keys()):
            pred = predictions[image_id]
            image_id = int(image_id)
            if image_id in self._seen:
                continue
            self._seen.add(image_id)
            self.img_ids.append(image_id)
            if pred is None or len(pred) == 0:
                self._preds.append((image_id, None, None, None))
            else:
                self._preds.append((image_id, pred['boxes'], pred['scores'], pred['labels']))

    def synchronize_between_processes(self, process_group=None):
        """Every rank ends with every rank's detections; an image id seen on several ranks keeps its FIRST occurrence in rank order."""
        from .dataparallel import collectives_active
        if not collectives_active(process_group):
            return
        device = next((b.device for _, b, _, _ in self._preds if b is not None), None)
        mine = [(i, None, None, None) if b is None else (i, b.detach().cpu(), s.detach().cpu(), l.detach().cpu()) for i, b, s, l in self._preds]
        merged, seen = [], set()
        for part in all_gather_picklable(mine, process_group):
            for rec in part:
                if rec[0] not in seen:
                    seen.add(rec[0])
                    merged.append(rec)
        if device is not None and device.type == 'cuda':
            merged = [(i, None, None, None) if b is None else (i, b.to(device), s.to(device), l.to(device)) for i, b, s, l in merged]
        self._preds, self._seen = merged, seen
        self.img_ids = [rec[0] for rec in merged]

    # ------------------------------------------------------------------------------------------------------------ accumulate
    def _ground_truth(self, img_ids):
        """-> (boxes f64 [M,4], area f64 [M], crowd u8 [M], offsets int64 [I*K+1]) with the annotations of (image i, category k) at
        offsets[i*K+k] .. in annotation order."""
        K = len(self.cat_ids)
        rows, keys = [], []
        for i, image_id in enumerate(img_ids):
            for rec in self._gt.get(image_id, ()):
                rows.append(rec[1:])
                keys.append(i * K + rec[0])
        rows = np.array(rows, dtype=np.float64).reshape(-1, 6)
        keys = np.array(keys, dtype=np.int64)
        order = np.argsort(keys, kind='stable')
        rows, keys = rows[order], keys[order]
        offsets = np.searchsorted(keys, np.arange(len(img_ids) * K + 1), side='left').astype(np.int64)
        return np.ascontiguousarray(rows[:, :4]), np.ascontiguousarray(rows[:, 4]), rows[:, 5].astype(np.uint8), offsets

    def _sorted_detections(self, preds, device):
        """The buffered detections of `preds` (ascending image id) on `device`, grouped into (image, category) segments in processing
        order -> dict of tensors; no synchronisation."""
        I, K = len(preds), len(self.cat_ids)
        boxes = [b.detach().reshape(-1, 4).to(device=device, dtype=torch.float32) for _, b, _, _ in preds if b is not None]
        scores = [s.detach().reshape(-1).to(device=device, dtype=torch.float32) for _, b, s, _ in preds if b is not None]
        labels = [l.detach().reshape(-1).to(device=device, dtype=torch.int64) for _, b, _, l in preds if b is not None]
        counts = [0 if b is None else int(b.shape[0]) for _, b, _, _ in preds]      # (shapes live on the host)
        boxes = torch.cat(boxes) if boxes else torch.zeros((0, 4), dtype=torch.float32, device=device)
        scores = torch.cat(scores) if scores else torch.zeros(0, dtype=torch.float32, device=device)
        labels = torch.cat(labels) if labels else torch.zeros(0, dtype=torch.int64, device=device)
        N = int(boxes.shape[0])
        img = torch.repeat_interleave(torch.arange(I, dtype=torch.int64), torch.tensor(counts, dtype=torch.int64)).to(device)
        # (x1, y1, f32(x2 - x1), f32(y2 - y1)) widened to f64: convert_to_xywh on f32 tensors, then .tolist()
        xywh = torch.cat((boxes[:, :2], boxes[:, 2:] - boxes[:, :2]), 1).to(torch.float64)
        cat_ids = torch.tensor(self.cat_ids, dtype=torch.int64, device=device)
        if K:
            k = torch.searchsorted(cat_ids, labels).clamp_(max=K - 1)
            k = torch.where(cat_ids[k] == labels, k, torch.full_like(k, K))      # K: a label outside the categories
        else:
            k = torch.zeros_like(labels)
        key = torch.where(k < K, img * K + k, torch.full_like(k, I * K))          # dropped detections sort behind every segment
        by_score = torch.sort(scores, descending=True, stable=True)[1]
        order = by_score[torch.sort(key[by_score], stable=True)[1]]
        key, k = key[order], k[order]
        det_off = torch.searchsorted(key, torch.arange(I * K + 1, dtype=torch.int64, device=device))
        rank = torch.arange(N, dtype=torch.int64, device=device) - det_off[key.clamp(max=max(I * K - 1, 0))] if N else key
        scores = scores[order]
        # per category: the segments' detections, images ascending and in-segment order kept, stable-sorted by descending score
        by_score = torch.sort(scores, descending=True, stable=True)[1]
        cat_order = by_score[torch.sort(k[by_score], stable=True)[1]]
        cat_off = torch.searchsorted(k[cat_order].contiguous(), torch.arange(K + 1, dtype=torch.int64, device=device))
        return {'xywh': xywh[order].contiguous(), 'det_off': det_off, 'rank': rank, 'cat_order': cat_order, 'cat_off': cat_off, 'N': N}

    def accumulate(self):
        preds = sorted(self._preds, key=lambda rec: rec[0])
        img_ids = [rec[0] for rec in preds]
        I, K = len(img_ids), len(self.cat_ids)
        devices = set(b.device for _, b, _, _ in preds if b is not None)
        on_hip = bool(devices) and all(d.type == 'cuda' for d in devices) and hip.host_policy.coco_eval_hip
        device = next(iter(devices)) if on_hip else torch.device('cpu')
        det = self._sorted_detections(preds, device)
        gt_box, gt_area, gt_crowd, gt_off = self._ground_truth(img_ids)
        if on_hip:
            precision, recall = self._accumulate_hip(det, gt_box, gt_area, gt_crowd, gt_off, I, K, device)
        else:
            precision, recall = self._accumulate_host(det, gt_box, gt_area, gt_crowd, gt_off, I, K)
        for ev in self.coco_eval.values():
            ev.eval = {'counts': [len(IOU_THRS), len(REC_THRS), K, len(AREA_RNG), len(MAX_DETS)], 'precision': precision, 'recall': recall}
            ev.path = 'hip' if on_hip else 'host'
            ev.img_ids = img_ids

    def _accumulate_hip(self, det, gt_box, gt_area, gt_crowd, gt_off, I, K, device):
        if K == 0:
            return (np.zeros((len(IOU_THRS), len(REC_THRS), 0, len(AREA_RNG), len(MAX_DETS))),
                    np.zeros((len(IOU_THRS), 0, len(AREA_RNG), len(MAX_DETS))))
        if max(det['N'], len(gt_area), I * K + 1) >= 2 ** 31:
            raise ValueError('coco evaluation: {} detections, {} images x {} categories exceed 32-bit offsets'.format(det['N'], I, K))

        def up(a, dtype=None):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(device)
        flags, npig = hip.coco_match(det['xywh'], up(gt_box), up(gt_area), up(gt_crowd), det['det_off'].to(torch.int32), up(gt_off, np.int32),
                                     up(IOU_THRS), up(AREA_RNG))
        npig = npig.view(I, K, len(AREA_RNG)).sum(0, dtype=torch.int64).to(torch.int32)
        precision, recall = hip.coco_accumulate(det['cat_order'].to(torch.int32), det['cat_off'].to(torch.int32), flags, det['rank'].to(torch.int32),
                                                npig, up(REC_THRS), up(np.array(MAX_DETS, dtype=np.int32)))
        return precision.cpu().numpy(), recall.cpu().numpy()

    # ------------------------------------------------------------------------------------------------------------ host path
    def _accumulate_host(self, det, gt_box, gt_area, gt_crowd, gt_off, I, K):
        T, R, A, M = len(IOU_THRS), len(REC_THRS), len(AREA_RNG), len(MAX_DETS)
        xywh = det['xywh'].cpu().numpy()
        det_off, rank = det['det_off'].cpu().numpy(), det['rank'].cpu().numpy()
        cat_order, cat_off = det['cat_order'].cpu().numpy(), det['cat_off'].cpu().numpy()
        N = det['N']
        matched = np.zeros((N, A, T), dtype=bool)
        ignored = np.zeros((N, A, T), dtype=bool)
        gt_ign = (gt_crowd[None, :] != 0) | (gt_area[None, :] < AREA_RNG[:, :1]) | (gt_area[None, :] > AREA_RNG[:, 1:])      # [A, n_gt]
        npig = np.zeros((max(K, 1), A), dtype=np.int64)
        if K and len(gt_area):
            seg_of_gt = np.repeat(np.arange(I * K), np.diff(gt_off))
            for a in range(A):
                npig[:K, a] = np.bincount(seg_of_gt % K, weights=~gt_ign[a], minlength=K).astype(np.int64)
        first = np.minimum(IOU_THRS, 1 - 1e-10)
        for seg in np.nonzero(np.diff(det_off))[0]:
            d0, d1, g0, g1 = det_off[seg], det_off[seg + 1], gt_off[seg], gt_off[seg + 1]
            d, g, crowd = xywh[d0:d1], gt_box[g0:g1], gt_crowd[g0:g1] != 0
            d_area = d[:, 2] * d[:, 3]
            # IoU of every pair, each operation rounded once
            w = np.minimum((d[:, 0] + d[:, 2])[:, None], (g[:, 0] + g[:, 2])[None]) - np.maximum(d[:, 0][:, None], g[:, 0][None])
            h = np.minimum((d[:, 1] + d[:, 3])[:, None], (g[:, 1] + g[:, 3])[None]) - np.maximum(d[:, 1][:, None], g[:, 1][None])
            inter = w * h
            union = np.where(crowd[None], np.broadcast_to(d_area[:, None], inter.shape), d_area[:, None] + (g[:, 2] * g[:, 3])[None] - inter)
            with np.errstate(divide='ignore', invalid='ignore'):
                iou = np.where((w <= 0) | (h <= 0), 0.0, inter / union)
            for a in range(A):
                ig = gt_ign[a, g0:g1]
                walk = np.argsort(ig, kind='stable')      # non-ignored first
                taken = np.zeros((T, g1 - g0), dtype=bool)
                lanes = np.arange(T)
                for di in range(d1 - d0):
                    best = first.copy()
                    m = np.full(T, -1)
                    live = np.ones(T, dtype=bool)
                    for gi in walk:
                        if ig[gi]:      # a non-ignored match is not given up for an ignored ground truth
                            live = ~((m >= 0) & ~ig[np.maximum(m, 0)])
                        move = live & ~(taken[:, gi] & ~crowd[gi]) & ~(iou[di, gi] < best)
                        best[move] = iou[di, gi]
                        m[move] = gi
                    hit = m >= 0
                    taken[lanes[hit], m[hit]] = True
                    matched[d0 + di, a] = hit
                    out = (d_area[di] < AREA_RNG[a, 0]) | (d_area[di] > AREA_RNG[a, 1])
                    ignored[d0 + di, a] = np.where(hit, ig[np.maximum(m, 0)], out) if len(ig) else out
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        for k in range(K):
            idx = cat_order[cat_off[k]:cat_off[k + 1]]
            for a in range(A):
                if npig[k, a] == 0:
                    continue
                for mi, max_det in enumerate(MAX_DETS):
                    sel = idx[rank[idx] < max_det]
                    mt, ign = matched[sel, a].T, ignored[sel, a].T      # [T, n]
                    tps = np.cumsum(mt & ~ign, axis=1).astype(np.float64)
                    fps = np.cumsum(~mt & ~ign, axis=1).astype(np.float64)
                    for t in range(T):
                        tp, fp = tps[t], fps[t]
                        rc = tp / npig[k, a]
                        pr = tp / (fp + tp + np.spacing(1))
                        recall[t, k, a, mi] = rc[-1] if len(tp) else 0
                        pr = np.maximum.accumulate(pr[::-1])[::-1]
                        at = np.searchsorted(rc, REC_THRS, side='left')
                        q = np.zeros(R)
                        ok = at < len(tp)
                        q[ok] = pr[at[ok]]
                        precision[t, :, k, a, mi] = q
        return precision, recall

    def summarize(self):
        for iou_type, ev in self.coco_eval.items():
            print('IoU metric: {}'.format(iou_type))
            ev.summarize()


def coco_gt_from_dataset(dataset):
    """The COCO dictionary of a detection dataset: `dataset.coco.dataset` where the dataset (under any number of `Subset`s) wraps a COCO
    index; otherwise the dataset is walked once -- per sample `(image, target)` with target `boxes` (xyxy), `labels`, `area`, `iscrowd`,
    `image_id` -- into images / annotations (boxes as xywh, annotation ids from 1) / categories (the labels seen, ascending)."""
    while isinstance(dataset, torch.utils.data.Subset):
        dataset = dataset.dataset
    coco = getattr(dataset, 'coco', None)
    if coco is not None:
        return coco if isinstance(coco, dict) else coco.dataset
    out = {'images': [], 'categories': [], 'annotations': []}
    seen = set()
    for index in range(len(dataset)):
        image, target = dataset[index]
        image_id = int(target['image_id'])
        out['images'].append({'id': image_id, 'height': int(image.shape[-2]), 'width': int(image.shape[-1])})
        boxes = torch.as_tensor(target['boxes']).reshape(-1, 4).clone()
        boxes[:, 2:] -= boxes[:, :2]
        rows = zip(boxes.tolist(), torch.as_tensor(target['labels']).tolist(), torch.as_tensor(target['area']).tolist(),
                   torch.as_tensor(target['iscrowd']).tolist())
        for box, label, area, crowd in rows:
            seen.add(label)
            out['annotations'].append({'image_id': image_id, 'bbox': box, 'category_id': label, 'area': area, 'iscrowd': crowd,
                                       'id': len(out['annotations']) + 1})
    out['categories'] = [{'id': label} for label in sorted(seen)]
    return out


class CocoDictDetection(torch.utils.data.Dataset):
    """A detection dataset over a COCO dictionary alone: sample i is (a seeded noise image of `images[i]`'s height x width, the target
    dict torchvision's detection models use -- boxes xyxy f32, labels, area, iscrowd, image_id).  What the evaluation entry runs on
    where the COCO images are absent (`--json '{"datasets": {"coco2017/val": {"coco_gt": <dictionary or path>}}}'`); `.coco.dataset`
    is the dictionary, so `coco_gt_from_dataset` hands it back unchanged."""

    class _Index(object):
        def __init__(self, dataset):
            self.dataset = dataset

    def __init__(self, coco_gt, seed=0):
        self.coco = self._Index(_gt_dict(coco_gt))
        self.seed = seed
        self._anns = {}
        for ann in self.coco.dataset['annotations']:
            self._anns.setdefault(ann['image_id'], []).append(ann)

    def __len__(self):
        return len(self.coco.dataset['images'])

    def __getitem__(self, index):
        info = self.coco.dataset['images'][index]
        anns = self._anns.get(info['id'], [])
        image = torch.rand(3, int(info['height']), int(info['width']), generator=torch.Generator().manual_seed(self.seed + index))
        boxes = torch.tensor([a['bbox'] for a in anns], dtype=torch.float32).reshape(-1, 4)
        boxes[:, 2:] += boxes[:, :2]
        return image, {'boxes': boxes, 'labels': torch.tensor([a['category_id'] for a in anns], dtype=torch.int64),
                       'area': torch.tensor([a['area'] for a in anns], dtype=torch.float32),
                       'iscrowd': torch.tensor([int(a.get('iscrowd', 0)) for a in anns], dtype=torch.int64),
                       'image_id': torch.tensor([int(info['id'])])}
