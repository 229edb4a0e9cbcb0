"""The data side of `configs/coco2017/**`: the COCO 2017 detection dataset, its (image, target) transforms and the aspect-ratio
grouped batch sampler, under the names of the reference's task scripts (script/task/coco/dataset.py, script/task/custom/sampler.py;
`config.resolve` maps `coco.dataset.*` and `custom.sampler.*` here).  Host Python over Pillow, numpy and torch alone: neither
pycocotools nor torchvision is needed.  What is restated from memory of those two packages is marked [recalled].

* `COCO` -- the part of pycocotools' index the dataset and the evaluation read [recalled]: `dataset`, `imgs`, `anns`, `cats`,
  `imgToAnns`, `getAnnIds(imgIds=, iscrowd=None)`, `loadAnns`, `loadImgs`; annotation order is file order.
* `CocoDetection` / `CustomCocoDetection` -- torchvision's dataset [recalled] and the reference's subclass.  Nothing touches the disk
  at construction: the annotation file is read on first use (`len`, indexing, `.coco`, `.ids`), so a config whose dataset directory is
  absent still PARSES and raises FileNotFoundError when the dataset is used, as `config.ImageFolder` and `config.VOCSegmentation` do.
* `Compose`, `ImageToTensor`, `CocoRandomHorizontalFlip`, `ConvertCocoPolysToMask4Detect` -- the pair transforms.  `Compose.plan`
  hands out a `transforms.DeferredDetSample` (source bytes + the drawn flip) in place of the float tensor where the chain is the
  loader's own; `transforms.coco_collate_fn` packs those into a `DeferredDetBatch` and `detection.GeneralizedRCNNTransform` finishes
  it on the device (csrc/det_input.hip).
* `GroupedBatchSampler`, `create_aspect_ratio_groups` & co. -- the `batch_sampler` of every COCO training loader.
Masks are NOT produced (see `ConvertCocoPolysToMask4Detect`), and `is_segment=True` is refused.
"""
import bisect
import json
import os
import random
from collections import defaultdict

import numpy as np
import torch
import torch.utils.data
from torch.utils.data.sampler import BatchSampler, Sampler

from .config import Placeholder
from .transforms import DeferredDetSample, to_tensor


# ------------------------------------------------------------------------------------------------------------ the index
class COCO(object):
    """pycocotools.coco.COCO as far as a detection dataset and its evaluation read it [recalled].  `annotation_file`: a path to the
    JSON, or the dictionary itself; None leaves an empty index (set `.dataset`, call `createIndex()`)."""

    def __init__(self, annotation_file=None):
        self.dataset, self.anns, self.cats, self.imgs = dict(), dict(), dict(), dict()
        self.imgToAnns, self.catToImgs = defaultdict(list), defaultdict(list)
        if annotation_file is not None:
            if isinstance(annotation_file, dict):
                dataset = annotation_file
            else:
                with open(os.path.expanduser(str(annotation_file))) as f:
                    dataset = json.load(f)
            if not isinstance(dataset, dict):
                raise ValueError('annotation file format {} not supported'.format(type(dataset)))
            self.dataset = dataset
            self.createIndex()

    def createIndex(self):
        anns, cats, imgs = dict(), dict(), dict()
        imgToAnns, catToImgs = defaultdict(list), defaultdict(list)
        for ann in self.dataset.get('annotations', ()):      # file order
            imgToAnns[ann['image_id']].append(ann)
            anns[ann['id']] = ann
            if 'category_id' in ann:
                catToImgs[ann['category_id']].append(ann['image_id'])
        for img in self.dataset.get('images', ()):
            imgs[img['id']] = img
        for cat in self.dataset.get('categories', ()):
            cats[cat['id']] = cat
        self.anns, self.cats, self.imgs, self.imgToAnns, self.catToImgs = anns, cats, imgs, imgToAnns, catToImgs

    def getAnnIds(self, imgIds=(), iscrowd=None):
        """ids of the annotations of the given image id(s) (all annotations when none is given), in file order; `iscrowd` 0 / 1 keeps
        those of that flag only"""
        img_ids = list(imgIds) if isinstance(imgIds, (list, tuple)) else [imgIds]
        if len(img_ids) == 0:
            anns = self.dataset.get('annotations', [])
        else:
            anns = [ann for img_id in img_ids if img_id in self.imgToAnns for ann in self.imgToAnns[img_id]]
        if iscrowd is not None:
            anns = [ann for ann in anns if ann['iscrowd'] == iscrowd]
        return [ann['id'] for ann in anns]

    def loadAnns(self, ids=()):
        return [self.anns[i] for i in ids] if isinstance(ids, (list, tuple)) else [self.anns[ids]]

    def loadImgs(self, ids=()):
        return [self.imgs[i] for i in ids] if isinstance(ids, (list, tuple)) else [self.imgs[ids]]


# --------------------------------------------------------------------------------------------------------- the datasets
class CocoDetection(torch.utils.data.Dataset):
    """torchvision.datasets.CocoDetection [recalled]: ids sorted, sample = (the image opened with Pillow and converted to RGB, the list
    of its annotations), then `transforms(image, target)` or `transform(image)` / `target_transform(target)`.  The annotation file is
    read on first use."""

    def __init__(self, root, annFile, transform=None, target_transform=None, transforms=None):
        self.root = None if root is None else os.path.expanduser(str(root))
        self.ann_file = annFile
        self.transform, self.target_transform, self.transforms = transform, target_transform, transforms
        self._coco = None
        self._ids = None

    def _index(self):
        if self._coco is None:
            path = self.ann_file
            if not isinstance(path, dict):
                path = os.path.expanduser(str(path))
                if not os.path.isfile(path):
                    raise FileNotFoundError('CocoDetection: annotation file {} does not exist (nothing is downloaded here)'.format(path))
            self._coco = COCO(path)
            self._ids = list(sorted(self._coco.imgs.keys()))
        return self._coco

    @property
    def coco(self):
        return self._index()

    @property
    def ids(self):
        self._index()
        return self._ids

    def _load_image(self, image_id):
        from PIL import Image
        path = self.coco.loadImgs(image_id)[0]['file_name']
        return Image.open(os.path.join(self.root or '', path)).convert('RGB')

    def _load_target(self, image_id):
        return self.coco.loadAnns(self.coco.getAnnIds(image_id))

    def _pair(self, index):
        image_id = self.ids[index]
        return self._load_image(image_id), self._load_target(image_id)

    def __getitem__(self, index):
        image, target = self._pair(index)
        if self.transforms is not None:
            return self.transforms(image, target)
        if self.transform is not None:
            image = self.transform(image)
        if self.target_transform is not None:
            target = self.target_transform(target)
        return image, target

    def __len__(self):
        return len(self.ids)


class CustomCocoDetection(CocoDetection):
    """The reference's subclass: the target is {image_id, annotations}, then `additional_transforms(image, target)`.  Where those can
    plan the sample (`Compose.plan`) and `hip.host_policy.det_input_hip` is on, the image comes back as a
    `transforms.DeferredDetSample` -- no pixel is touched here; with the switch off the workers convert as before."""

    def __init__(self, img_folder, ann_file, transforms=None):
        super().__init__(img_folder, ann_file)
        self.additional_transforms = transforms

    def __getitem__(self, index):
        image, annotations = self._pair(index)
        target = {'image_id': self.ids[index], 'annotations': annotations}
        chain = self.additional_transforms
        if chain is None:
            return image, target
        plan = getattr(chain, 'plan', None)
        if plan is not None:
            from . import hip
            planned = plan(image, target) if hip.host_policy.det_input_hip else None
            if planned is not None:
                return planned
        return chain(image, target)


# ------------------------------------------------------------------------------------------------------- the transforms
# COCO's 17 person keypoints: the nose, then (left, right) pairs of eyes, ears, shoulders, elbows, wrists, hips, knees, ankles
_KEYPOINT_MIRROR = [0] + [k + 1 if k % 2 else k - 1 for k in range(1, 17)]


def _flip_coco_person_keypoints(kps, width):
    """keypoints [n,17,3] (x, y, visibility) of the mirrored image: left and right joints change places, x -> width - x, and a joint
    of visibility 0 stays all zero (COCO's convention)"""
    mirrored = kps[:, _KEYPOINT_MIRROR].clone()
    mirrored[..., 0] = width - mirrored[..., 0]
    mirrored[mirrored[..., 2] == 0] = 0
    return mirrored


class ImageToTensor(object):
    """ToTensor of the image; `jpeg_quality`: through Pillow's JPEG first, on the host."""

    def __init__(self, jpeg_quality=None):
        self.jpeg_quality = jpeg_quality

    def __call__(self, image, target):
        if self.jpeg_quality is None:
            return to_tensor(image), target
        from io import BytesIO
        from PIL import Image
        coded = BytesIO()
        image.save(coded, 'JPEG', quality=self.jpeg_quality)
        return to_tensor(Image.open(coded)), target


def _flip_target(target, width):
    """the target side of `CocoRandomHorizontalFlip`, in place: box x -> width - x with the two corners changing places, masks
    mirrored, person keypoints through `_flip_coco_person_keypoints`"""
    boxes = target['boxes']
    left, right = width - boxes[:, 2], width - boxes[:, 0]
    boxes[:, 0], boxes[:, 2] = left, right
    if 'masks' in target:
        target['masks'] = target['masks'].flip(-1)
    if 'keypoints' in target:
        target['keypoints'] = _flip_coco_person_keypoints(target['keypoints'], width)
    return target


class CocoRandomHorizontalFlip(object):
    """With probability `prob` (one `random.random()` per sample) the tensor image and its target are mirrored."""

    def __init__(self, prob):
        self.prob = prob

    def draw(self):
        return random.random() < self.prob

    def __call__(self, image, target):
        if not self.draw():
            return image, target
        return image.flip(-1), _flip_target(target, image.shape[-1])


class ConvertCocoPolysToMask4Detect(object):
    """{image_id, annotations} -> the target dict of torchvision's detection models: crowd annotations dropped, `boxes` xywh -> xyxy and
    clamped to the image, `labels`, `image_id`, `keypoints` where the annotations carry them, all under the keep-mask of the boxes that
    are not degenerate, and `area` / `iscrowd` of the non-crowd annotations for the conversion to a COCO index.
    The target has NO `masks` key: rasterising the polygons needs pycocotools' mask routines, which are not available here, Faster R-CNN
    never reads masks, and nothing in this tree could verify a rasteriser of its own."""

    def __call__(self, image, target):
        width, height = image.size
        objects = [a for a in target['annotations'] if a['iscrowd'] == 0]
        n = len(objects)
        xywh = torch.tensor([a['bbox'] for a in objects], dtype=torch.float32).reshape(n, 4)
        x0, y0 = xywh[:, 0], xywh[:, 1]
        x1, y1 = x0 + xywh[:, 2], y0 + xywh[:, 3]
        boxes = torch.stack([x0.clamp(0, width), y0.clamp(0, height), x1.clamp(0, width), y1.clamp(0, height)], dim=1)
        proper = (boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])      # a box the clamp left with no width or height goes
        converted = {'boxes': boxes[proper],
                     'labels': torch.tensor([a['category_id'] for a in objects], dtype=torch.int64)[proper],
                     'image_id': torch.tensor([target['image_id']])}
        if n and 'keypoints' in objects[0]:
            joints = torch.tensor([a['keypoints'] for a in objects], dtype=torch.float32)
            converted['keypoints'] = joints.reshape(n, -1, 3)[proper]
        # (of every non-crowd annotation, the improper boxes included: the reference's conversion to a COCO index reads them so)
        converted['area'] = torch.tensor([a['area'] for a in objects])
        converted['iscrowd'] = torch.tensor([a['iscrowd'] for a in objects])
        return image, converted


class Compose(object):
    """The pair transforms one after the other: each takes and returns (image, target)."""

    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, image, target):
        pair = (image, target)
        for step in self.transforms:
            pair = step(*pair)
        return pair

    def _flat(self):
        """the transforms with nested `Compose`s spread out"""
        out = []
        for step in self.transforms:
            out += step._flat() if isinstance(step, Compose) else [step]
        return out

    def _chain(self):
        """(the transforms in front that read the image's size only, the flip or None) when the chain, nested `Compose`s flattened, is
        [ConvertCocoPolysToMask4Detect ...] -> ImageToTensor(jpeg_quality=None) -> [CocoRandomHorizontalFlip], else None"""
        ts = self._flat()
        pre = []
        while ts and type(ts[0]) is ConvertCocoPolysToMask4Detect:
            pre.append(ts.pop(0))
        if not ts or type(ts[0]) is not ImageToTensor or ts[0].jpeg_quality is not None:
            return None
        ts.pop(0)
        flip = ts.pop(0) if ts and type(ts[0]) is CocoRandomHorizontalFlip else None
        return None if ts else (pre, flip)

    def plan(self, image, target):
        """The loader's own chain on an 8-bit RGB image: the target as `__call__` gives it (boxes flipped on the host), the same draws in
        the same order, and a `DeferredDetSample` (source bytes, flip) in place of the float tensor -- no pixel is touched.  Any other
        chain or input: None, and nothing is drawn."""
        from PIL import Image
        chain = self._chain()
        if chain is None or not isinstance(image, Image.Image) or image.mode != 'RGB' or min(image.size) < 1:
            return None
        pre, flip = chain
        for t in pre:
            image, target = t(image, target)
        flipped = flip.draw() if flip is not None else False
        if flipped:
            target = _flip_target(target, image.size[0])
        return DeferredDetSample(np.asarray(image), flipped), target


# ---------------------------------------------------------------------------------------------- filtering, construction
def _box_is_empty(annotation):
    """a box whose width or height is at most one pixel"""
    _, _, w, h = annotation['bbox']
    return w <= 1 or h <= 1


def has_only_empty_bbox(anno):
    """True when no annotation of the image has a box of more than one pixel both ways"""
    return all(_box_is_empty(a) for a in anno)


def count_visible_keypoints(anno):
    """keypoints of the image whose visibility flag (every third number) is above zero"""
    return sum(int(flag > 0) for a in anno for flag in a['keypoints'][2::3])


def has_valid_annotation(anno, min_keypoints_per_image=10):
    """An image counts as annotated when it has an annotation with a box that is not empty; a keypoint dataset (the first annotation
    carries `keypoints`) also asks for `min_keypoints_per_image` visible keypoints in the image."""
    if not anno or has_only_empty_bbox(anno):
        return False
    return 'keypoints' not in anno[0] or count_visible_keypoints(anno) >= min_keypoints_per_image


class _AnnotatedSubset(torch.utils.data.Subset):
    """The `Subset` of the images with a valid annotation; its indices are worked out from the index on first use."""

    def __init__(self, dataset, cat_list=None):
        self.dataset = dataset
        self.cat_list = cat_list
        self._indices = None

    def _annotated(self, image_id):
        coco = self.dataset.coco
        anno = coco.loadAnns(coco.getAnnIds(imgIds=image_id, iscrowd=None))
        if self.cat_list:
            anno = [a for a in anno if a['category_id'] in self.cat_list]
        return has_valid_annotation(anno)

    @property
    def indices(self):
        if self._indices is None:
            self._indices = [position for position, image_id in enumerate(self.dataset.ids) if self._annotated(image_id)]
        return self._indices


def remove_images_without_annotations(dataset, cat_list=None):
    """-> the `Subset` of a `CocoDetection` whose images have a valid annotation (of the categories in `cat_list`, if given).  The
    subset is worked out on first use, so that a dataset whose files are absent can still be constructed."""
    if not isinstance(dataset, CocoDetection):
        raise TypeError('remove_images_without_annotations: a CocoDetection is required, got {}'.format(type(dataset).__name__))
    return _AnnotatedSubset(dataset, cat_list)


def convert_to_coco_api(ds):
    """Any detection dataset of (image, target) pairs walked once -> a `COCO` index: one image record per sample (its id from
    `image_id`, its size from the image), one annotation per box -- xyxy back to xywh, `category_id` from `labels`, `area`, `iscrowd`,
    `keypoints` / `num_keypoints` where the target has them -- with ids counted from 1 (an id of 0 reads as "unmatched" in COCO's
    evaluation), and the categories = the labels seen, ascending.  Masks are not encoded: there are none here.  No target is changed."""
    images, annotations, labels_seen = [], [], set()
    for position in range(len(ds)):
        image, target = ds[position]
        image_id = int(target['image_id'].item())
        images.append({'id': image_id, 'height': image.shape[-2], 'width': image.shape[-1]})
        corners = target['boxes']
        xywh = torch.cat([corners[:, :2], corners[:, 2:] - corners[:, :2]], dim=1).tolist()
        fields = {'category_id': target['labels'].tolist(), 'area': target['area'].tolist(), 'iscrowd': target['iscrowd'].tolist()}
        joints = target['keypoints'].flatten(1).tolist() if 'keypoints' in target else None
        for k, box in enumerate(xywh):
            record = {'id': len(annotations) + 1, 'image_id': image_id, 'bbox': box}
            record.update({name: values[k] for name, values in fields.items()})
            if joints is not None:
                record['keypoints'] = joints[k]
                record['num_keypoints'] = sum(1 for flag in joints[k][2::3] if flag != 0)
            labels_seen.add(record['category_id'])
            annotations.append(record)
    index = COCO()
    index.dataset = {'images': images, 'categories': [{'id': label} for label in sorted(labels_seen)], 'annotations': annotations}
    index.createIndex()
    return index


def get_coco_api_from_dataset(dataset):
    """-> the `COCO` index of a dataset (its `.dataset` is the dictionary `coco_eval.CocoBoxEvaluator` takes): the dataset's own where
    a `CocoDetection` lies under its `Subset`s, else the one `convert_to_coco_api` builds from the samples"""
    inner = dataset
    while isinstance(inner, torch.utils.data.Subset) and not isinstance(inner, CocoDetection):
        inner = inner.dataset
    return inner.coco if isinstance(inner, CocoDetection) else convert_to_coco_api(dataset)


def get_coco(img_dir_path, ann_file_path, transforms, annotated_only, is_segment):
    """`CustomCocoDetection` with `ConvertCocoPolysToMask4Detect` in front of `transforms`, filtered to the annotated images if asked"""
    if is_segment:
        raise NotImplementedError('coco_dataset(is_segment=True) rasterises the polygons with pycocotools, which is not available here')
    chain = [ConvertCocoPolysToMask4Detect()] + ([] if transforms is None else [transforms])
    dataset = CustomCocoDetection(img_dir_path, ann_file_path, transforms=Compose(chain))
    return remove_images_without_annotations(dataset) if annotated_only else dataset


def coco_dataset(img_dir_path, ann_file_path, annotated_only, random_horizontal_flip=None, is_segment=False, transforms=None,
                 jpeg_quality=None):
    """The dataset every `configs/coco2017/**` file names.  Without `transforms` the chain is `ImageToTensor(jpeg_quality)` and, for
    detection with a flip probability, `CocoRandomHorizontalFlip`.  Nothing is read at construction."""
    if transforms is None:
        flips = random_horizontal_flip is not None and not is_segment
        transforms = Compose([ImageToTensor(jpeg_quality)] + ([CocoRandomHorizontalFlip(random_horizontal_flip)] if flips else []))
    return get_coco(img_dir_path, ann_file_path, transforms, annotated_only, is_segment)


# --------------------------------------------------------------------------------------------------------- the sampler
BATCH_SAMPLER_DICT = dict()


def register_batch_sampler(cls):
    BATCH_SAMPLER_DICT[cls.__name__] = cls
    return cls


@register_batch_sampler
class GroupedBatchSampler(BatchSampler):
    """Batches of `batch_size` indices of ONE group each, over another sampler: `group_ids[i]`, an integer in [0, num_groups), is the
    group of sample i.  A batch goes out as soon as its group has gathered `batch_size` indices, so the order follows the sampler's as
    closely as the grouping allows.  `len()` is `len(sampler) // batch_size` whatever the groups are: when the sampler is exhausted and
    batches are still owed, the groups with the most indices waiting go first, each topped up from the start of what the sampler gave
    for that group in this pass; what is left after that is dropped."""

    def __init__(self, sampler, group_ids, batch_size):
        if not isinstance(sampler, Sampler):
            raise ValueError('GroupedBatchSampler: a torch.utils.data.Sampler is required, got {!r}'.format(sampler))
        self.sampler, self.group_ids, self.batch_size = sampler, group_ids, batch_size

    def __len__(self):
        return len(self.sampler) // self.batch_size

    def __iter__(self):
        size, owed = self.batch_size, len(self)
        waiting, given = dict(), dict()      # group -> indices not yet in a batch / every index of this pass, in the sampler's order
        for index in self.sampler:
            group = self.group_ids[index]
            given.setdefault(group, []).append(index)
            batch = waiting.setdefault(group, [])
            batch.append(index)
            if len(batch) == size:
                del waiting[group]
                owed -= 1
                yield batch
        # (the sort is stable: of two groups with as many indices waiting, the one that started waiting first goes first)
        for group, batch in sorted(waiting.items(), key=lambda item: -len(item[1])):
            if owed <= 0:
                break
            batch = batch + given[group][:size - len(batch)]
            if len(batch) != size:
                raise RuntimeError('GroupedBatchSampler: group {} has {} samples, fewer than a batch needs to be topped up'.format(
                    group, len(given[group])))
            owed -= 1
            yield batch


def compute_aspect_ratios(dataset, indices=None):
    """width / height of every sample (of `indices`): from `get_height_and_width(i)` where the dataset has it, from the COCO index for
    a `CocoDetection` (no image is opened), through its indices for a `Subset`; any other dataset is walked sample by sample.  A
    torchdistill dataset wrapper is looked through (`org_dataset`)."""
    data = getattr(dataset, 'org_dataset', dataset)
    sized = hasattr(data, 'get_height_and_width')
    if isinstance(data, torch.utils.data.Subset) and not sized:
        positions = range(len(data)) if indices is None else indices
        return compute_aspect_ratios(data.dataset, [data.indices[p] for p in positions])
    if indices is None:
        indices = range(len(data))
    if sized:
        sizes = (data.get_height_and_width(i) for i in indices)
    elif isinstance(data, CocoDetection):
        records = (data.coco.imgs[data.ids[i]] for i in indices)
        sizes = ((record['height'], record['width']) for record in records)
    else:
        sizes = (data[i][0].shape[-2:] for i in indices)
    return [float(width) / float(height) for height, width in sizes]


def _quantize(x, bins):
    """the number of bin edges at or below each value (the edges in any order): a value on an edge falls into the bin to its right"""
    edges = sorted(bins)
    return [bisect.bisect_right(edges, value) for value in x]


def create_aspect_ratio_groups(dataset, aspect_ratio_group_factor=0):
    """The group id of every sample: its aspect ratio quantised by the 2k + 1 edges 2 ** linspace(-1, 1, 2k + 1) (the single edge 1.0
    at k = 0).  A dataset that is a `Placeholder` or whose files are absent leaves a `Placeholder`, so that the config still parses."""
    k = aspect_ratio_group_factor
    if not isinstance(dataset, Placeholder):
        try:
            edges = np.power(2.0, np.linspace(-1, 1, 2 * k + 1)).tolist() if k > 0 else [1.0]
            return _quantize(compute_aspect_ratios(dataset), edges)
        except FileNotFoundError:
            pass
    return Placeholder('custom.sampler.create_aspect_ratio_groups', (), dict(dataset=dataset, aspect_ratio_group_factor=k))


# what `config.resolve` hands out under `coco.dataset.<name>` and `custom.sampler.<name>`
__all__ = ['COCO', 'CocoDetection', 'CustomCocoDetection', 'Compose', 'ImageToTensor', 'CocoRandomHorizontalFlip',
           'ConvertCocoPolysToMask4Detect', 'has_only_empty_bbox', 'count_visible_keypoints', 'has_valid_annotation',
           'remove_images_without_annotations', 'convert_to_coco_api', 'get_coco_api_from_dataset', 'get_coco', 'coco_dataset',
           'GroupedBatchSampler', 'compute_aspect_ratios', 'create_aspect_ratio_groups']
