"""CPU: the COCO data side (sc2-benchmark_amd/coco_data.py): the grouped batch sampler on hand-worked cases, the aspect-ratio groups,
the dataset over a small COCO directory, the conversion to a COCO index, and the reference's COCO config with the datasets absent and
present."""
import json
import os
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import SequentialSampler, Subset

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import det_input_cases as DC  # noqa: E402

REF = '/root/reference/configs'
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason='reference tree not present (GPU box)')
COCO_YAML = os.path.join(REF, 'coco2017/supervised_compression/entropic_student',
                         'faster_rcnn_splittable_resnet50-fp-beta0.08_fpn_from_faster_rcnn_resnet50_fpn.yaml')


# ------------------------------------------------------------------------------------------------------------ the sampler
def test_grouped_batch_sampler_hand_worked(S):
    from sc2bench_amd.coco_data import GroupedBatchSampler
    group_ids = [0, 0, 1, 0, 1, 1, 0]
    sampler = SequentialSampler(range(7))
    # batch size 2: 0, 1 fill group 0; 2, 4 fill group 1; 3, 6 fill group 0 again; 5 stays behind: 7 // 2 = 3 batches are out already
    two = GroupedBatchSampler(sampler, group_ids, 2)
    assert len(two) == 3 and list(two) == [[0, 1], [2, 4], [3, 6]]
    assert list(two) == [[0, 1], [2, 4], [3, 6]]      # a second epoch starts from empty buffers
    # batch size 3: group 0 fills at 3, group 1 at 5; 6 stays behind
    three = GroupedBatchSampler(sampler, group_ids, 3)
    assert len(three) == 2 and list(three) == [[0, 1, 3], [2, 4, 5]]
    # batch size 5: nothing fills (group 0 holds 0, 1, 3, 6, group 1 holds 2, 4, 5); 7 // 5 = 1 batch is owed: the fullest buffer is
    # refilled from the front of its own group's samples
    five = GroupedBatchSampler(sampler, group_ids, 5)
    assert len(five) == 1 and list(five) == [[0, 1, 3, 6, 0]]
    # batch size 4 over six samples of which group 1 has four: group 1 fills at index 5... and one more batch is not owed
    assert list(GroupedBatchSampler(SequentialSampler(range(6)), [0, 1, 1, 0, 1, 1], 4)) == [[1, 2, 4, 5]]
    with pytest.raises(ValueError, match='Sampler'):
        GroupedBatchSampler([0, 1, 2], group_ids, 2)
    assert S.coco_data.BATCH_SAMPLER_DICT['GroupedBatchSampler'] is GroupedBatchSampler


class _Sized(torch.utils.data.Dataset):
    def __init__(self, hws):
        self.hws = hws

    def __len__(self):
        return len(self.hws)

    def get_height_and_width(self, i):
        return self.hws[i]

    def __getitem__(self, i):
        raise AssertionError('the aspect ratios must come from get_height_and_width')


def test_create_aspect_ratio_groups(S):
    from sc2bench_amd import coco_data as D
    from sc2bench_amd.config import Placeholder
    # (height, width): ratios 0.4, 0.5, 0.7, 1.0, 2.0, 3.0
    data = _Sized([(10, 4), (10, 5), (10, 7), (8, 8), (5, 10), (5, 15)])
    assert D.compute_aspect_ratios(data) == [0.4, 0.5, 0.7, 1.0, 2.0, 3.0]
    assert D.create_aspect_ratio_groups(data) == [0, 0, 0, 1, 1, 1]      # k = 0: one bin edge at 1.0, and 1.0 itself goes right
    bins = (2 ** np.linspace(-1, 1, 7)).tolist()
    assert bins[0] == 0.5 and bins[3] == 1.0 and bins[6] == 2.0
    # k = 3: edges 0.5, 0.63, 0.79, 1, 1.26, 1.59, 2; a ratio exactly on an edge goes right
    assert D.create_aspect_ratio_groups(data, aspect_ratio_group_factor=3) == [0, 1, 2, 4, 7, 7]
    assert D._quantize([0.49, 0.5, 1.99, 2.0], [2.0, 0.5]) == [0, 1, 1, 2]      # (the bins are sorted first)
    assert D.create_aspect_ratio_groups(Subset(data, [4, 0, 3]), aspect_ratio_group_factor=3) == [7, 0, 4]
    assert D.compute_aspect_ratios(Subset(data, [4, 0, 3]), [2, 0]) == [1.0, 2.0]
    # a dataset that is not there: the config must still parse
    absent = D.coco_dataset('/nonexistent/train2017', '/nonexistent/instances.json', annotated_only=True, random_horizontal_flip=0.5)
    for dataset in (absent, Placeholder('torchvision.datasets.Nothing')):
        groups = D.create_aspect_ratio_groups(dataset, aspect_ratio_group_factor=3)
        assert isinstance(groups, Placeholder) and groups.key == 'custom.sampler.create_aspect_ratio_groups'
        assert groups.kwargs['aspect_ratio_group_factor'] == 3
    with pytest.raises(FileNotFoundError, match='instances.json'):
        len(absent)
    with pytest.raises(FileNotFoundError):
        absent.dataset.coco


def test_aspect_ratios_of_a_coco_dataset_open_no_image(S, tmp_path):
    from sc2bench_amd import coco_data as D
    ann = tmp_path / 'instances.json'
    ann.write_text(json.dumps({'images': DC.COCO_IMAGES, 'annotations': DC.COCO_ANNOTATIONS, 'categories': DC.COCO_CATEGORIES}))
    data = D.coco_dataset(str(tmp_path / 'no_images_here'), str(ann), annotated_only=False)
    assert D.compute_aspect_ratios(data) == [24 / 36, 1.0, 40 / 30]      # ids 3, 5, 7
    annotated = D.coco_dataset(str(tmp_path / 'no_images_here'), str(ann), annotated_only=True)
    assert D.create_aspect_ratio_groups(annotated, aspect_ratio_group_factor=3) == [2, 5]


# ------------------------------------------------------------------------------------------------------------- the index
def test_coco_index(S):
    from sc2bench_amd.coco_data import COCO
    coco = COCO({'images': DC.COCO_IMAGES, 'annotations': DC.COCO_ANNOTATIONS, 'categories': DC.COCO_CATEGORIES})
    assert sorted(coco.imgs) == [3, 5, 7] and sorted(coco.anns) == [11, 12, 13, 14, 15] and sorted(coco.cats) == [1, 2]
    assert coco.getAnnIds(imgIds=7) == [11, 13, 14, 15] == coco.getAnnIds(imgIds=[7], iscrowd=None)      # file order
    assert coco.getAnnIds(imgIds=7, iscrowd=0) == [11, 14, 15] and coco.getAnnIds(imgIds=7, iscrowd=1) == [13]
    assert coco.getAnnIds(imgIds=5) == [] and coco.getAnnIds() == [11, 12, 13, 14, 15]
    assert [a['id'] for a in coco.loadAnns([15, 11])] == [15, 11] and coco.loadAnns(12)[0]['image_id'] == 3
    assert coco.loadImgs(3)[0]['file_name'] == 'three.png' and [i['id'] for i in coco.loadImgs([7, 5])] == [7, 5]
    assert [a['id'] for a in coco.imgToAnns[7]] == [11, 13, 14, 15]
    empty = COCO()
    assert empty.dataset == {} and empty.getAnnIds() == []


# ----------------------------------------------------------------------------------------------------------- the dataset
def _unplanned(dataset):
    """the same dataset with planning switched off: the float tensors of the host chain"""
    inner = dataset.dataset if isinstance(dataset, Subset) else dataset
    inner.additional_transforms.plan = None
    return dataset


def test_dataset_over_a_coco_directory(S, tmp_path):
    from sc2bench_amd import coco_data as D
    img_dir, ann_file = DC.write_coco(tmp_path)
    data = _unplanned(D.coco_dataset(img_dir, ann_file, annotated_only=False))
    assert isinstance(data, D.CustomCocoDetection) and isinstance(data, D.CocoDetection)
    assert data.ids == [3, 5, 7] and len(data) == 3
    image, target = data[2]
    assert image.dtype == torch.float32 and tuple(image.shape) == (3, 30, 40)
    assert torch.equal(image[0], image[1]) and torch.equal(image[1], image[2])      # the grey file, converted to RGB
    assert torch.equal(image[0], torch.from_numpy(DC.source(30, 40, seed=7)[:, :, 0]).float().div(255))
    assert sorted(target) == ['area', 'boxes', 'image_id', 'iscrowd', 'labels'] and 'masks' not in target
    # the crowd annotation is dropped; xywh -> xyxy; the box past the edge is clamped to 40 x 30; the zero-width box is masked out
    assert target['boxes'].dtype == torch.float32 and target['boxes'].tolist() == [[2.0, 3.0, 12.0, 15.0], [30.0, 20.0, 40.0, 30.0]]
    assert target['labels'].dtype == torch.int64 and target['labels'].tolist() == [2, 1]
    assert target['image_id'].tolist() == [7]
    assert target['area'].tolist() == [120.0, 0.0, 750.0] and target['iscrowd'].tolist() == [0, 0, 0]      # of the non-crowd annotations
    _, empty = data[1]      # the image without annotations
    assert tuple(empty['boxes'].shape) == (0, 4) and empty['labels'].numel() == 0 and empty['image_id'].tolist() == [5]
    annotated = D.coco_dataset(img_dir, ann_file, annotated_only=True)
    assert isinstance(annotated, Subset) and len(annotated) == 2 and list(annotated.indices) == [0, 2]
    assert [int(annotated[i][1]['image_id']) for i in range(2)] == [3, 7]
    with pytest.raises(NotImplementedError, match='pycocotools'):
        D.coco_dataset(img_dir, ann_file, annotated_only=False, is_segment=True)
    # the plain CocoDetection: the target is the annotation list
    image, anns = D.CocoDetection(img_dir, ann_file)[2]
    assert image.mode == 'RGB' and image.size == (40, 30) and [a['id'] for a in anns] == [11, 13, 14, 15]


def test_annotation_filters(S):
    from sc2bench_amd import coco_data as D
    box = lambda w, h, **k: dict({'bbox': [0, 0, w, h]}, **k)      # noqa: E731
    assert D.has_only_empty_bbox([box(1, 10), box(10, 0.5)]) and not D.has_only_empty_bbox([box(1, 10), box(2, 2)])
    assert not D.has_valid_annotation([]) and not D.has_valid_annotation([box(1, 1)]) and D.has_valid_annotation([box(5, 5)])
    kp = lambda n: box(5, 5, keypoints=[1, 1, 2] * n + [0, 0, 0] * (17 - n))      # noqa: E731
    assert D.count_visible_keypoints([kp(4), kp(5)]) == 9
    assert not D.has_valid_annotation([kp(4), kp(5)]) and D.has_valid_annotation([kp(4), kp(6)])


def test_flip_maps_boxes_with_width_minus_x(S):
    from sc2bench_amd import coco_data as D
    image = torch.arange(24, dtype=torch.float32).reshape(1, 2, 12).repeat(3, 1, 1)
    target = {'boxes': torch.tensor([[1.0, 0.0, 4.0, 2.0], [0.0, 1.0, 12.0, 2.0]])}
    out, flipped = D.CocoRandomHorizontalFlip(1.0)(image, target)
    assert torch.equal(out, image.flip(-1)) and flipped['boxes'].tolist() == [[8.0, 0.0, 11.0, 2.0], [0.0, 1.0, 12.0, 2.0]]
    same, kept = D.CocoRandomHorizontalFlip(0.0)(image, {'boxes': torch.tensor([[1.0, 0.0, 4.0, 2.0]])})
    assert same is image and kept['boxes'].tolist() == [[1.0, 0.0, 4.0, 2.0]]


# ------------------------------------------------------------------------------------------------- evaluation and config
def test_coco_api_from_dataset_feeds_the_box_evaluator(S, tmp_path):
    from sc2bench_amd import coco_data as D
    img_dir, ann_file = DC.write_coco(tmp_path)
    data = D.coco_dataset(img_dir, ann_file, annotated_only=True)
    api = D.get_coco_api_from_dataset(data)      # through the Subset: the dataset's own index
    assert api is data.dataset.coco and api.dataset['categories'] == DC.COCO_CATEGORIES
    evaluator = S.coco_eval.CocoBoxEvaluator(api)
    assert evaluator.cat_ids == [1, 2] and sorted(evaluator._gt) == [3, 7]
    assert S.coco_eval.coco_gt_from_dataset(data) is api.dataset
    # a dataset without an index is walked: boxes back to xywh, annotation ids from 1
    listed = [data[i] for i in range(len(data))]
    walked = D.get_coco_api_from_dataset(listed)
    assert isinstance(walked, D.COCO) and [i['id'] for i in walked.dataset['images']] == [3, 7]
    assert walked.dataset['images'][1] == {'id': 7, 'height': 30, 'width': 40}
    assert [a['bbox'] for a in walked.dataset['annotations']] == [[4.0, 6.0, 12.0, 20.0], [2.0, 3.0, 10.0, 12.0], [30.0, 20.0, 10.0, 10.0]]
    assert [a['id'] for a in walked.dataset['annotations']] == [1, 2, 3] and walked.dataset['categories'] == [{'id': 1}, {'id': 2}]
    assert listed[1][1]['boxes'].tolist() == [[2.0, 3.0, 12.0, 15.0], [30.0, 20.0, 40.0, 30.0]]      # the walk changed no target
    assert S.coco_eval.CocoBoxEvaluator(walked).cat_ids == [1, 2]


def test_build_data_loader_with_a_batch_sampler(S, tmp_path):
    from sc2bench_amd import coco_data as D, evaluation as E
    from sc2bench_amd.config import Placeholder
    img_dir, ann_file = DC.write_coco(tmp_path)
    data = D.coco_dataset(img_dir, ann_file, annotated_only=False)
    block = {'dataset_id': 'coco', 'sampler': {'class_or_func': SequentialSampler, 'kwargs': None},
             'batch_sampler': {'key': 'GroupedBatchSampler', 'kwargs': {'batch_size': 2, 'group_ids': [0, 1, 0]}},
             'collate_fn': 'coco_collate_fn', 'kwargs': {'num_workers': 0, 'batch_size': 7}}
    loader = E.build_data_loader({'coco': data}, block)
    assert isinstance(loader.batch_sampler, D.GroupedBatchSampler) and loader.batch_size is None and len(loader) == 1
    (images, targets), = list(loader)
    assert isinstance(images, S.transforms.DeferredDetBatch) and images.sizes == [(36, 24), (30, 40)]
    assert [int(t['image_id']) for t in targets] == [3, 7]
    with pytest.raises(KeyError, match='NoSuchSampler'):
        E.build_data_loader({'coco': data}, dict(block, batch_sampler={'key': 'NoSuchSampler'}))
    with pytest.raises(ValueError, match='group_ids'):
        E.build_data_loader({'coco': data}, dict(block, batch_sampler={'key': 'GroupedBatchSampler', 'kwargs': {
            'batch_size': 2, 'group_ids': Placeholder('custom.sampler.create_aspect_ratio_groups')}}))
    plain = E.build_data_loader({'coco': data}, {k: v for k, v in block.items() if k != 'batch_sampler'})      # no batch sampler: as before
    assert plain.batch_size == 7 and isinstance(plain.sampler, SequentialSampler) and isinstance(loader.batch_sampler.sampler, SequentialSampler)


@needs_ref
def test_reference_coco_config_with_the_datasets_absent(S):
    from sc2bench_amd import config as C, coco_data as D
    assert C.resolve('coco.dataset.coco_dataset') is D.coco_dataset
    assert C.resolve('custom.sampler.create_aspect_ratio_groups') is D.create_aspect_ratio_groups
    assert C.resolve('torchvision.datasets.CocoDetection') is C.ImageFolder      # what existing keys resolve to does not change
    cfg = C.load_yaml_file(COCO_YAML)
    train, val = cfg['datasets']['coco2017/train'], cfg['datasets']['coco2017/val']
    assert isinstance(train, Subset) and isinstance(train.dataset, D.CustomCocoDetection) and isinstance(val, D.CustomCocoDetection)
    flat = train.dataset.additional_transforms._flat()
    assert [type(t).__name__ for t in flat] == ['ConvertCocoPolysToMask4Detect', 'ImageToTensor', 'CocoRandomHorizontalFlip']
    assert flat[2].prob == 0.5 and [type(t).__name__ for t in val.additional_transforms._flat()] == ['ConvertCocoPolysToMask4Detect', 'ImageToTensor']
    sampler = cfg['train']['stage1']['train_data_loader']['batch_sampler']
    assert sampler['key'] == 'GroupedBatchSampler' and sampler['kwargs']['batch_size'] == 6
    assert isinstance(sampler['kwargs']['group_ids'], C.Placeholder)


@needs_ref
def test_reference_coco_config_pointed_at_a_directory(S, tmp_path):
    from sc2bench_amd import config as C, coco_data as D, evaluation as E
    root = tmp_path / 'datasets' / 'coco2017'
    for split in ('train', 'val'):
        DC.write_coco(root, image_dir='{}2017'.format(split), ann_path='annotations/instances_{}2017.json'.format(split))
    text = open(COCO_YAML).read()
    assert "'~/datasets/'" in text
    path = tmp_path / 'coco.yaml'
    path.write_text(text.replace("'~/datasets/'", "'{}/'".format(tmp_path / 'datasets')))
    cfg = C.load_yaml_file(str(path))
    block = cfg['train']['stage2']['train_data_loader']
    assert block['batch_sampler']['kwargs']['group_ids'] == [2, 5]      # 24 x 36 and 40 x 30 among the bins of k = 3
    C.overwrite_config(block, {'batch_sampler': {'kwargs': {'batch_size': 1}}, 'kwargs': {'num_workers': 0}})
    loader = E.build_data_loader(cfg['datasets'], block)
    assert isinstance(loader.batch_sampler, D.GroupedBatchSampler) and isinstance(loader.batch_sampler.sampler, torch.utils.data.RandomSampler)
    batches = list(loader)
    assert len(batches) == 2 and sorted(int(t[0]['image_id']) for _, t in batches) == [3, 7]
    assert all(isinstance(images, S.transforms.DeferredDetBatch) and len(images) == 1 for images, _ in batches)
    test_loader = E.build_data_loader(cfg['datasets'], dict(cfg['test']['test_data_loader'], kwargs={'batch_size': 1, 'num_workers': 0}))
    assert [int(t[0]['image_id']) for _, t in test_loader] == [3, 5, 7]
