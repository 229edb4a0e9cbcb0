"""Shared by tests/test_seg_augment_cpu.py and tests/test_gpu_seg_augment.py: seeded sources, the PASCAL chains at test size, a small
VOC tree, and the batch a list of explicit sample parameters gives (reference tensors from tests/ref_pil_resize.py)."""
import os
import random

import numpy as np
import torch

import ref_pil_resize as ref

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def source(h, w, seed=0, classes=21):
    """-> (uint8 [h,w,3], uint8 [h,w] with the values 0 .. classes-1 and 255)"""
    rng = np.random.RandomState(1000 * h + w + seed)
    mask = rng.randint(0, classes + 1, (h, w)).astype(np.uint8)
    mask[mask == classes] = 255
    return rng.randint(0, 256, (h, w, 3)).astype(np.uint8), mask


def sample(T, image, mask, nh, nw, flip=False, top=0, left=0, out=None):
    """A `DeferredSegSample` with explicit parameters: `out` = crop size (the train form, padded to at least that) or None (evaluation)."""
    if out is None:
        return T.DeferredSegSample(image, mask, nh, nw, flip, 0, 0, nh, nw, nh, nw, MEAN, STD)
    return T.DeferredSegSample(image, mask, nh, nw, flip, top, left, out, out, max(nh, out), max(nw, out), MEAN, STD)


def reference_batch(samples):
    """What the host chain and the collate function give for these samples, from the numpy restatement: (float32 [n,3,H,W], int64 [n,H,W])"""
    H, W = max(s.out_h for s in samples), max(s.out_w for s in samples)
    images = torch.zeros((len(samples), 3, H, W), dtype=torch.float32)
    targets = torch.full((len(samples), H, W), 255, dtype=torch.int64)
    for i, s in enumerate(samples):
        x, t = ref.augment(s.image, s.mask, s.nh, s.nw, s.flip, s.top, s.left, s.out_h, s.out_w, s.pad_h, s.pad_w, s.mean, s.std)
        images[i, :, :s.out_h, :s.out_w] = torch.from_numpy(x)
        targets[i, :s.out_h, :s.out_w] = torch.from_numpy(t)
    return images, targets


def train_chain(T, min_size=20, max_size=90, crop=33, p=0.5):
    return T.CustomCompose([T.CustomRandomResize(min_size, max_size), T.CustomRandomHorizontalFlip(p), T.CustomRandomCrop(crop),
                            T.CustomToTensor(), T.CustomNormalize(MEAN, STD)])


def eval_chain(T, size=40):
    return T.CustomCompose([T.CustomRandomResize(size, size), T.CustomToTensor(converts_sample=True, converts_target=True),
                            T.CustomNormalize(MEAN, STD)])


VOC_SIZES = ((37, 50), (50, 37), (33, 33))


def write_voc_tree(root, classes=5):
    """root/VOCdevkit/VOC2012 with three images (JPEG) and palette masks (PNG, values 0 .. classes-1 and 255), train.txt and val.txt"""
    from PIL import Image
    base = os.path.join(str(root), 'VOCdevkit', 'VOC2012')
    for d in ('JPEGImages', 'SegmentationClass', os.path.join('ImageSets', 'Segmentation')):
        os.makedirs(os.path.join(base, d))
    ids = []
    for k, (h, w) in enumerate(VOC_SIZES):
        image, mask = source(h, w, seed=k, classes=classes)
        name = '2012_{:06d}'.format(k)
        Image.fromarray(image).save(os.path.join(base, 'JPEGImages', name + '.jpg'), quality=95)
        pal = Image.fromarray(mask, mode='L').convert('P')
        pal.putpalette([v for i in range(256) for v in (i, (7 * i) % 256, 255 - i)])
        pal.save(os.path.join(base, 'SegmentationClass', name + '.png'))
        ids.append(name)
    for split in ('train', 'val'):
        with open(os.path.join(base, 'ImageSets', 'Segmentation', split + '.txt'), 'w') as f:
            f.write('\n'.join(ids) + '\n')
    return ids


def seed_all(seed):
    random.seed(seed)
    torch.manual_seed(seed)
