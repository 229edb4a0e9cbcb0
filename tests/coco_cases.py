"""Inputs of the COCO box-AP tests: the hand-worked cases of tests/test_coco_ref_cpu.py and seeded random sets on a coarse grid
(equal scores, duplicate boxes and IoUs exactly on a threshold occur).  Every case is (gt dictionary, predictions) with
predictions {image id: {'boxes' f32 [n,4] xyxy, 'scores' f32 [n], 'labels' int64 [n]}} as numpy arrays."""
import numpy as np


def ann(image_id, cat, x, y, w, h, area=None, crowd=0):
    return {'image_id': image_id, 'category_id': cat, 'bbox': [float(x), float(y), float(w), float(h)],
            'area': float(w * h if area is None else area), 'iscrowd': crowd}


def gt_dict(anns, cats=(1,), images=None):
    anns = [dict(a, id=i + 1) for i, a in enumerate(anns)]
    images = sorted(set(a['image_id'] for a in anns)) if images is None else images
    return {'images': [{'id': i, 'height': 512, 'width': 512} for i in images], 'annotations': anns, 'categories': [{'id': c} for c in cats]}


def pred(rows):
    """rows: [(x, y, w, h, score, label)] -> one image's prediction (boxes as xyxy)"""
    rows = np.array(rows, dtype=np.float64).reshape(-1, 6)
    boxes = np.stack([rows[:, 0], rows[:, 1], rows[:, 0] + rows[:, 2], rows[:, 1] + rows[:, 3]], 1).astype(np.float32)
    return {'boxes': boxes, 'scores': rows[:, 4].astype(np.float32), 'labels': rows[:, 5].astype(np.int64)}


def perfect():
    boxes = {1: [(0, 0, 10, 10), (100, 100, 50, 50)], 2: [(20, 20, 200, 200), (300, 300, 20, 20)]}
    gt = gt_dict([ann(i, 1, *b) for i, bs in boxes.items() for b in bs])
    return gt, {i: pred([b + (0.9 - 0.1 * j, 1) for j, b in enumerate(bs)]) for i, bs in boxes.items()}


def tp_fp_tp():
    gt = gt_dict([ann(1, 1, 0, 0, 100, 100), ann(1, 1, 200, 200, 100, 100)])
    return gt, {1: pred([(0, 0, 100, 100, .9, 1), (400, 400, 100, 100, .8, 1), (200, 200, 100, 100, .7, 1)])}


def crowd_twice():
    gt = gt_dict([ann(1, 1, 0, 0, 200, 200, crowd=1), ann(1, 1, 300, 300, 100, 100)])
    return gt, {1: pred([(10, 10, 50, 50, .9, 1), (100, 100, 50, 50, .8, 1), (300, 300, 100, 100, .7, 1)])}


def absorbed_by_out_of_range_gt():
    # the first annotation's box is small (900) but its `area` FIELD is medium (2000): the field decides
    gt = gt_dict([ann(1, 1, 0, 0, 30, 30, area=2000), ann(1, 1, 100, 100, 10, 10)])
    return gt, {1: pred([(0, 0, 30, 30, .9, 1), (100, 100, 10, 10, .8, 1)])}


def small_unmatched_in_large():
    gt = gt_dict([ann(1, 1, 0, 0, 100, 100)])
    return gt, {1: pred([(300, 300, 10, 10, .9, 1), (0, 0, 100, 100, .5, 1)])}


def equal_iou_later_gt():
    gt = gt_dict([ann(1, 1, 0, 0, 100, 100), ann(1, 1, 0, 0, 100, 100)])
    return gt, {1: pred([(0, 0, 100, 100, .9, 1), (0, 0, 100, 100, .8, 1)])}


def keep_non_ignored_match():
    # the detection overlaps the plain ground truth with IoU 0.6 and lies inside the crowd (IoU 1 against a crowd)
    gt = gt_dict([ann(1, 1, 0, 0, 10, 6), ann(1, 1, 0, 0, 50, 50, crowd=1)])
    return gt, {1: pred([(0, 0, 10, 10, .9, 1)])}


def cut_to_100():
    gt = gt_dict([ann(1, 1, 0, 0, 100, 100)])
    rows = [(200 + 2 * i, 300, 20, 20, 0.99 - 0.001 * i, 1) for i in range(100)] + [(0, 0, 100, 100, 0.01, 1)]
    return gt, {1: pred(rows)}


def max_det_cuts():
    boxes = [(40 * i, 0, 30, 30) for i in range(11)]
    gt = gt_dict([ann(1, 1, *b) for b in boxes])
    return gt, {1: pred([b + (0.95 - 0.01 * i, 1) for i, b in enumerate(boxes)])}


def image_without_predictions():
    gt = gt_dict([ann(1, 1, 0, 0, 100, 100), ann(2, 1, 0, 0, 100, 100)])
    return gt, {1: pred([(0, 0, 100, 100, .9, 1)]), 2: {}}


def category_without_gt():
    gt = gt_dict([ann(1, 1, 0, 0, 100, 100)], cats=(1, 2))
    return gt, {1: pred([(0, 0, 100, 100, .9, 1), (0, 0, 100, 100, .95, 2)])}


def label_outside_categories():
    gt = gt_dict([ann(1, 1, 0, 0, 100, 100)], cats=(1, 3))
    return gt, {1: pred([(0, 0, 100, 100, .99, 99), (0, 0, 100, 100, .98, 2), (0, 0, 100, 100, .9, 1), (0, 0, 100, 100, .97, 0)])}


def iou_on_threshold():
    gt = gt_dict([ann(1, 1, 0, 0, 100, 100)])
    return gt, {1: pred([(0, 0, 100, 50, .9, 1)])}


HAND_CASES = (perfect, tp_fp_tp, crowd_twice, absorbed_by_out_of_range_gt, small_unmatched_in_large, equal_iou_later_gt,
              keep_non_ignored_match, cut_to_100, max_det_cuts, image_without_predictions, category_without_gt, label_outside_categories,
              iou_on_threshold)


def random_boxes(rng, n, grid=8, side=16):
    """n xywh boxes with corners on a `grid`-pixel lattice: duplicates, nested boxes of half the area, IoUs of 1/2, 3/4, 2/3 ... occur"""
    xy = rng.randint(0, side, size=(n, 2)) * grid
    wh = rng.randint(1, 9, size=(n, 2)) * grid
    return np.concatenate([xy, wh], 1).astype(np.float64)


def random_case(seed, images=6, cats=(1, 2, 5), max_gt=6, max_det=12, crowd=0.15, empty=0.2, big_segment=0):
    """A seeded set: scores from ten values (ties), labels partly outside the categories, `area` fields that differ from the box area,
    crowds, images without predictions or without ground truth; `big_segment` > 0 gives image 0 / the first category that many ground
    truths and detections."""
    rng = np.random.RandomState(seed)
    anns, preds = [], {}
    labels = list(cats) + [max(cats) + 1]
    for i in range(images):
        image_id = 10 + 3 * i
        n_gt = 0 if rng.rand() < empty else rng.randint(1, max_gt + 1)
        for b in random_boxes(rng, n_gt):
            area = b[2] * b[3] * (1.0 if rng.rand() < 0.7 else rng.choice([0.25, 4.0, 40.0]))
            anns.append(ann(image_id, int(rng.choice(cats)), *b, area=area, crowd=int(rng.rand() < crowd)))
        if i == 0 and big_segment:
            for b in random_boxes(rng, big_segment):
                anns.append(ann(image_id, cats[0], *b, crowd=int(rng.rand() < crowd)))
        n_det = 0 if rng.rand() < empty else rng.randint(1, max_det + 1)
        rows = [tuple(b) + (rng.randint(1, 11) / 10.0, int(rng.choice(labels))) for b in random_boxes(rng, n_det)]
        # some detections copy a ground truth of their image exactly
        mine = [a for a in anns if a['image_id'] == image_id]
        for a in mine[:rng.randint(0, len(mine) + 1)]:
            rows.append(tuple(a['bbox']) + (rng.randint(1, 11) / 10.0, a['category_id']))
        if i == 0 and big_segment:
            rows += [tuple(b) + (rng.randint(1, 11) / 10.0, cats[0]) for b in random_boxes(rng, big_segment)]
        preds[image_id] = pred(rows) if rows else {}
    return gt_dict(anns, cats=cats, images=sorted(preds)), preds
