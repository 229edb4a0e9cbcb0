"""Shared inputs of the COCO data-side and sc2_det_input tests: seeded sources, a packed buffer, and a small COCO directory written
with Pillow."""
import json
import os

import numpy as np

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
ODD_MEAN, ODD_STD = [0.1, 0.5, 0.9], [0.3, 1.7, 0.05]


def source(h, w, seed=0):
    return np.random.RandomState(seed * 7919 + h * 131 + w).randint(0, 256, (h, w, 3), dtype=np.uint8)


def pack(sources, lead=0):
    """-> (flat u8 buffer with `lead` bytes of junk in front and the images back to back, [byte offsets])"""
    chunks, offsets, at = [np.full((lead,), 0xA5, dtype=np.uint8)], [], lead
    for src in sources:
        offsets.append(at)
        chunks.append(np.ascontiguousarray(src).reshape(-1))
        at += src.size
    return np.concatenate(chunks), offsets


def ceil_to(v, m):
    return -(-v // m) * m


# The COCO directory: image ids deliberately not in file order.
#   id 7  40 x 30 (w x h) grey       a plain box, a crowd box, a degenerate box (zero width), a box past the right / bottom edge
#   id 3  24 x 36                     one box
#   id 5  32 x 32                     no annotation
COCO_IMAGES = [{'id': 7, 'file_name': 'seven.png', 'width': 40, 'height': 30},
               {'id': 3, 'file_name': 'three.png', 'width': 24, 'height': 36},
               {'id': 5, 'file_name': 'five.png', 'width': 32, 'height': 32}]
COCO_ANNOTATIONS = [
    {'id': 11, 'image_id': 7, 'bbox': [2.0, 3.0, 10.0, 12.0], 'category_id': 2, 'area': 120.0, 'iscrowd': 0, 'segmentation': []},
    {'id': 12, 'image_id': 3, 'bbox': [4.0, 6.0, 12.0, 20.0], 'category_id': 1, 'area': 240.0, 'iscrowd': 0, 'segmentation': []},
    {'id': 13, 'image_id': 7, 'bbox': [1.0, 1.0, 20.0, 20.0], 'category_id': 1, 'area': 400.0, 'iscrowd': 1, 'segmentation': []},
    {'id': 14, 'image_id': 7, 'bbox': [5.0, 5.0, 0.0, 9.0], 'category_id': 2, 'area': 0.0, 'iscrowd': 0, 'segmentation': []},
    {'id': 15, 'image_id': 7, 'bbox': [30.0, 20.0, 25.0, 30.0], 'category_id': 1, 'area': 750.0, 'iscrowd': 0, 'segmentation': []},
]
COCO_CATEGORIES = [{'id': 1, 'name': 'one'}, {'id': 2, 'name': 'two'}]


def write_coco(root, image_dir='images', ann_path='annotations/instances.json'):
    """-> (image directory, annotation file) under `root`; image 7 is a grey ('L') file, the others RGB noise"""
    from PIL import Image
    img_dir, ann_file = os.path.join(str(root), image_dir), os.path.join(str(root), ann_path)
    os.makedirs(img_dir, exist_ok=True)
    os.makedirs(os.path.dirname(ann_file), exist_ok=True)
    for info in COCO_IMAGES:
        h, w = info['height'], info['width']
        if info['id'] == 7:
            Image.fromarray(source(h, w, seed=7)[:, :, 0], mode='L').save(os.path.join(img_dir, info['file_name']))
        else:
            Image.fromarray(source(h, w, seed=info['id']), mode='RGB').save(os.path.join(img_dir, info['file_name']))
    with open(ann_file, 'w') as f:
        json.dump({'images': COCO_IMAGES, 'annotations': COCO_ANNOTATIONS, 'categories': COCO_CATEGORIES}, f)
    return img_dir, ann_file
