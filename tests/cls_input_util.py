"""Shared by tests/test_cls_input_cpu.py and tests/test_gpu_cls_input.py: seeded sources, the two ImageNet chains as `config` builds them
from the keys and arguments every configs/ilsvrc2012/** file names, a small class-per-directory tree of PNG files, a small frozen
classifier, and the reference batch of explicit descriptors (tests/ref_cls_input.py)."""
import os
import random

import numpy as np
import torch

import ref_cls_input as RC

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def source(h, w, seed=0):
    return np.random.RandomState(1000 * h + w + seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _build(C, key, **kwargs):
    """what the loader's `!import_call` does with {key, init: {kwargs}}"""
    return C.resolve(key)(**kwargs)


def train_chain(C, size=(224, 224), p=0.5):
    """`ilsvrc2012/train` of configs/ilsvrc2012/**: RandomResizedCrop([224, 224]) -> RandomHorizontalFlip(0.5) -> ToTensor -> Normalize"""
    tv = 'torchvision.transforms.'
    return _build(C, tv + 'Compose', transforms=[
        _build(C, tv + 'RandomResizedCrop', size=list(size)), _build(C, tv + 'RandomHorizontalFlip', p=p), _build(C, tv + 'ToTensor'),
        _build(C, tv + 'Normalize', mean=list(MEAN), std=list(STD))])


def eval_chain(C, resize=256, crop=(224, 224)):
    """`ilsvrc2012/val`: Resize(256) -> CenterCrop([224, 224]) -> ToTensor -> Normalize"""
    tv = 'torchvision.transforms.'
    return _build(C, tv + 'Compose', transforms=[
        _build(C, tv + 'Resize', size=resize), _build(C, tv + 'CenterCrop', size=list(crop)), _build(C, tv + 'ToTensor'),
        _build(C, tv + 'Normalize', mean=list(MEAN), std=list(STD))])


TREE_SIZES = ((37, 53), (53, 37), (40, 40), (101, 77), (45, 160), (64, 48))      # (every one within ratio 4 of Resize(32))


def write_image_tree(root, classes=3, per_class=2):
    """root/<class>/<k>.png, lossless, sizes from TREE_SIZES in turn -> [(path, label)] in the dataset's order"""
    from PIL import Image
    out, k = [], 0
    for c in range(classes):
        d = os.path.join(str(root), 'class_{}'.format(c))
        os.makedirs(d)
        for j in range(per_class):
            h, w = TREE_SIZES[k % len(TREE_SIZES)]
            path = os.path.join(d, '{:03d}.png'.format(j))
            Image.fromarray(source(h, w, seed=k)).save(path)
            out.append((path, c))
            k += 1
    return out


class TinyClassifier(torch.nn.Module):
    """a small frozen classifier for any input size (f32, any device)"""

    def __init__(self, num_classes=6, seed=5):
        super().__init__()
        torch.manual_seed(seed)
        self.conv = torch.nn.Conv2d(3, 8, 3, stride=2, padding=1)
        self.fc = torch.nn.Linear(8, num_classes)
        for p in self.parameters():
            p.requires_grad_(False)

    def forward(self, x):
        return self.fc(torch.tanh(self.conv(x)).mean((2, 3)))


def stage_config():
    """a one-term stage: the student's output against the frozen teacher's, mean squared error"""
    return {
        'teacher': {'sequential': [], 'forward_hook': {'input': [], 'output': []}, 'requires_grad': False},
        'student': {'sequential': [], 'frozen_modules': [], 'forward_hook': {'input': [], 'output': []}, 'requires_grad': True},
        'optimizer': {'key': 'SGD', 'kwargs': {'lr': 0.01}},
        'criterion': {'key': 'WeightedSumLoss', 'kwargs': {'sub_terms': {'out': {
            'criterion': {'key': 'MSELoss', 'kwargs': {'reduction': 'sum'}},
            'criterion_wrapper': {'key': 'SimpleLossWrapper', 'kwargs': {
                'input': {'is_from_teacher': False, 'module_path': '.', 'io': 'output'},
                'target': {'is_from_teacher': True, 'module_path': '.', 'io': 'output'}}},
            'weight': 1.0}}}},
    }


def seed_all(seed):
    random.seed(seed)
    torch.manual_seed(seed)


# ------------------------------------------------------------------------------------------------ explicit samples for the kernel tests
def train_sample(T, image, top, left, ch, cw, oh, ow, flip=False):
    """the train form: the stored box is the crop, resized to the window"""
    box = np.ascontiguousarray(image[top:top + ch, left:left + cw])
    return T.DeferredClsSample(box, ch, cw, 0, 0, oh, ow, flip, 0, 0, oh, ow, MEAN, STD)


def eval_sample(T, image, size, oh, ow, trimmed=True):
    """the evaluation form: Resize(size) -> CenterCrop((oh, ow)) with the box trimmed to the taps"""
    _, box, f = RC.resize_center_crop(image, size, oh, ow, trimmed=trimmed)
    return T.DeferredClsSample(box, f['full_h'], f['full_w'], f['row0'], f['col0'], f['nh'], f['nw'], False, f['top'], f['left'], oh, ow,
                               MEAN, STD)


def reference(sample):
    """float32 [3, oh, ow] of one sample from the numpy restatement"""
    u8 = RC.window(np.asarray(sample.image), sample.full_h, sample.full_w, sample.row0, sample.col0, sample.nh, sample.nw, sample.flip,
                   sample.top, sample.left, sample.out_h, sample.out_w)
    return torch.from_numpy(RC.normalize(u8, sample.mean, sample.std))


def reference_batch(samples):
    return torch.stack([reference(s) for s in samples])
