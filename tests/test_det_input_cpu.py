"""CPU: planned COCO samples (`coco_data.Compose.plan` -> `transforms.DeferredDetSample` -> `coco_collate_fn` ->
`transforms.DeferredDetBatch`) against the unplanned chain: the same draws, the same tensors bit for bit, the same targets, the same
losses and detections; and what stays unplanned."""
import os
import pickle
import random
import sys

import numpy as np
import pytest
import torch
from torch.utils.data import Subset

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import det_input_cases as DC  # noqa: E402
import ref_det_train as RT  # noqa: E402


def _datasets(tmp_path, **kwargs):
    """(the dataset, the same dataset with planning switched off) over the small COCO directory"""
    from sc2bench_amd import coco_data as D
    img_dir, ann_file = DC.write_coco(tmp_path)
    planned = D.coco_dataset(img_dir, ann_file, **kwargs)
    plain = D.coco_dataset(img_dir, ann_file, **kwargs)
    (plain.dataset if isinstance(plain, Subset) else plain).additional_transforms.plan = None
    return planned, plain


def _same_target(a, b):
    return sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in a)


def test_planned_samples_make_the_same_draws_and_tensors(S, tmp_path):
    T = S.transforms
    planned, plain = _datasets(tmp_path, annotated_only=False, random_horizontal_flip=0.5)
    random.seed(11)
    got = [planned[i] for i in range(3)] + [planned[i] for i in range(3)]
    after_planned = random.random()
    random.seed(11)
    want = [plain[i] for i in range(3)] + [plain[i] for i in range(3)]
    assert random.random() == after_planned      # as many draws, from the same generator
    flips = [s.flip for s, _ in got]
    assert True in flips and False in flips
    for (sample, target), (image, want_target) in zip(got, want):
        assert isinstance(sample, T.DeferredDetSample) and sample.image.dtype == np.uint8
        assert sample.shape == tuple(image.shape) and sample.image.shape == (image.shape[1], image.shape[2], 3)
        host = sample.host()
        assert host.dtype == torch.float32 and torch.equal(host, image)
        assert _same_target(target, want_target)      # boxes flipped on the host already
    images, targets = T.coco_collate_fn(got)
    assert isinstance(images, T.DeferredDetBatch) and isinstance(targets, tuple) and len(images) == 6
    assert images.buf.dtype == torch.uint8 and images.buf.dim() == 1 and not images.buf.is_cuda
    assert images.sizes == [tuple(image.shape[-2:]) for image, _ in want] and images.flips == flips
    assert images.buf.numel() == sum(3 * h * w for h, w in images.sizes)
    for a, (b, _) in zip(images.tensors('cpu'), want):
        assert torch.equal(a, b)
    assert S.detection.original_sizes(images) == [tuple(image.shape[-2:]) for image, _ in want]
    # no flip configured: nothing is drawn
    planned0, _ = _datasets(tmp_path, annotated_only=False)
    random.seed(5)
    first = random.random()
    random.seed(5)
    assert planned0[0][0].flip is False and random.random() == first


def test_batch_slices_pickles_and_refuses_a_mix(S, tmp_path):
    T = S.transforms
    planned, plain = _datasets(tmp_path, annotated_only=False, random_horizontal_flip=0.5)
    random.seed(2)
    items = [planned[i] for i in range(3)]
    images, _ = T.coco_collate_fn(items)
    head = images[:2]
    assert isinstance(head, T.DeferredDetBatch) and len(head) == 2 and head.sizes == images.sizes[:2]
    for a, b in zip(head.tensors('cpu'), images.tensors('cpu')[:2]):
        assert torch.equal(a, b)
    tail = images[1:]
    assert torch.equal(tail.tensors('cpu')[1], images.tensors('cpu')[2]) and tail.offsets == images.offsets[1:]
    one = images[2]
    assert isinstance(one, T.DeferredDetSample) and one.flip == items[2][0].flip and np.array_equal(one.image, items[2][0].image)
    sample = pickle.loads(pickle.dumps(items[0][0]))
    assert isinstance(sample, T.DeferredDetSample) and sample.flip == items[0][0].flip and np.array_equal(sample.image, items[0][0].image)
    again = pickle.loads(pickle.dumps(images))
    assert again.sizes == images.sizes and torch.equal(again.buf, images.buf)
    assert images.to('cpu') is images and images.device == torch.device('cpu')
    from sc2bench_amd import training
    moved = training._to_device((images, [{'boxes': torch.zeros(1, 4)}]), torch.device('cpu'))      # what a distillation stage does
    assert moved[0] is images and torch.is_tensor(moved[1][0]['boxes'])
    if torch.cuda.is_available():      # (pinning needs a device's runtime)
        pinned = images.pin_memory()
        assert pinned is images and images.buf.is_pinned()
    assert callable(images.pin_memory)
    with pytest.raises(TypeError, match='mixes planned'):
        T.coco_collate_fn([items[0], plain[1]])
    # unplanned pairs: as before
    out = T.coco_collate_fn([plain[0], plain[1]])
    assert isinstance(out, tuple) and isinstance(out[0], tuple) and torch.is_tensor(out[0][0])


def test_other_chains_stay_unplanned(S, tmp_path):
    from sc2bench_amd import coco_data as D
    img_dir, ann_file = DC.write_coco(tmp_path)
    coded = D.coco_dataset(img_dir, ann_file, annotated_only=False, jpeg_quality=90)      # Pillow's JPEG on the host first
    image, target = coded[0]
    assert torch.is_tensor(image) and image.dtype == torch.float32 and tuple(image.shape) == (3, 36, 24)

    class Halve(object):
        def __call__(self, image, target):
            return image * 0.5, target

    foreign = D.coco_dataset(img_dir, ann_file, annotated_only=False, transforms=D.Compose([D.ImageToTensor(), Halve()]))
    image, _ = foreign[0]
    assert torch.is_tensor(image) and float(image.max()) <= 0.5
    assert D.Compose([D.ImageToTensor(), Halve()])._chain() is None and D.Compose([D.CocoRandomHorizontalFlip(0.5)])._chain() is None
    assert D.Compose([D.ImageToTensor(jpeg_quality=50)])._chain() is None
    pre, flip = D.Compose([D.ConvertCocoPolysToMask4Detect(), D.Compose([D.ImageToTensor(), D.CocoRandomHorizontalFlip(0.3)])])._chain()
    assert len(pre) == 1 and flip.prob == 0.3
    # an image that is not 8-bit RGB is not planned
    from PIL import Image
    chain = D.Compose([D.ImageToTensor()])
    assert chain.plan(Image.new('L', (4, 4)), {}) is None and chain.plan(torch.zeros(3, 4, 4), {}) is None
    sample, _ = chain.plan(Image.new('RGB', (5, 4)), {})
    assert sample.shape == (3, 4, 5)


def test_planning_follows_the_switch(S, tmp_path, monkeypatch):
    planned, _ = _datasets(tmp_path, annotated_only=False, random_horizontal_flip=0.5)
    random.seed(4)
    want = [planned[i] for i in range(3)]
    assert all(isinstance(image, S.transforms.DeferredDetSample) for image, _ in want)
    monkeypatch.setattr(S.hip.host_policy, 'det_input_hip', False)      # off: the workers convert, as before
    random.seed(4)
    got = [planned[i] for i in range(3)]
    for (image, target), (sample, want_target) in zip(got, want):
        assert torch.is_tensor(image) and torch.equal(image, sample.host()) and _same_target(target, want_target)


def test_transformed_needs_a_hip_device_and_tensors_are_converted_once(S):
    T = S.transforms
    batch = T.DeferredDetBatch([T.DeferredDetSample(DC.source(9, 13, seed=1), True), T.DeferredDetSample(DC.source(13, 9, seed=2), False)])
    tr = S.detection.GeneralizedRCNNTransform(16, 24, DC.MEAN, DC.STD)
    with pytest.raises(S.hip.Sc2Error, match='not a HIP device'):
        batch.transformed(tr, 'cpu')
    with pytest.raises(S.hip.Sc2Error, match='not a HIP device'):
        batch.transformed(tr)
    first, second = batch.tensors('cpu'), batch.tensors()
    assert first is not second and all(a is b for a, b in zip(first, second))      # the teacher's and the student's: one conversion
    assert batch[:1]._on_device is batch._on_device
    batch.release()
    assert all(a is not b and torch.equal(a, b) for a, b in zip(batch.tensors('cpu'), first))


def test_resolve_hands_out_the_restated_names_only(S):
    from sc2bench_amd import config as C, coco_data as D
    for name in D.__all__:
        prefix = 'custom.sampler.' if name in ('GroupedBatchSampler', 'compute_aspect_ratios', 'create_aspect_ratio_groups') else 'coco.dataset.'
        assert C.resolve(prefix + name) is getattr(D, name)
    for key in ('coco.dataset.os', 'coco.dataset.json', 'custom.sampler.np', 'custom.sampler.torch', 'coco.dataset._flip_target'):
        assert isinstance(C.resolve(key), C.Placeholder)


def test_transform_on_the_cpu_equals_the_list(S, tmp_path):
    planned, plain = _datasets(tmp_path, annotated_only=False, random_horizontal_flip=0.5)
    random.seed(3)
    images, targets = S.transforms.coco_collate_fn([planned[i] for i in range(3)])
    random.seed(3)
    want_images, want_targets = S.transforms.coco_collate_fn([plain[i] for i in range(3)])
    tr = S.detection.GeneralizedRCNNTransform(48, 80, DC.MEAN, DC.STD)
    before = S.transforms.DeferredDetBatch.launches
    got, got_t = tr(images, list(targets))
    want, want_t = tr(list(want_images), list(want_targets))
    assert S.transforms.DeferredDetBatch.launches == before      # no device: the present code on `tensors('cpu')`
    assert torch.equal(got.tensors, want.tensors) and got.image_sizes == want.image_sizes
    assert all(_same_target(a, b) for a, b in zip(got_t, want_t))
    assert all(torch.equal(a['boxes'], b['boxes']) for a, b in zip(targets, want_targets))      # the inputs were not changed


def test_training_detector_losses_are_bit_equal_for_the_planned_batch(S):
    T = S.transforms
    H, W = RT.STANDIN_IMAGE
    sources = [DC.source(H, W, seed=40), DC.source(H, W, seed=41)]
    batch = T.DeferredDetBatch([T.DeferredDetSample(sources[0], False), T.DeferredDetSample(sources[1], True)])
    listed = [T.to_tensor(sources[0]), T.to_tensor(sources[1]).flip(-1)]
    model = RT.standin_model(S.detection).train()
    torch.manual_seed(7)
    want = model(listed, RT.standin_targets())
    torch.manual_seed(7)
    got = model(batch, RT.standin_targets())
    assert sorted(got) == ['loss_box_reg', 'loss_classifier', 'loss_objectness', 'loss_rpn_box_reg']
    for k in want:
        assert torch.isfinite(got[k]) and torch.equal(got[k], want[k])


def test_evaluate_detection_is_the_same_for_planned_batches(S, tmp_path):
    from sc2bench_amd import evaluation as E
    planned, plain = _datasets(tmp_path, annotated_only=False)
    collate = S.transforms.COLLATE_FUNC_DICT['coco_collate_fn']
    model = RT.standin_model(S.detection)
    results = []
    for dataset in (planned, plain):
        loader = torch.utils.data.DataLoader(dataset, batch_size=2, collate_fn=collate)
        results.append(E.evaluate_detection(model, loader, torch.device('cpu'), max_samples=3))
    a, b = results
    assert a['samples'] == b['samples'] == 3 and a['evaluator'].img_ids == b['evaluator'].img_ids == [3, 5, 7]
    assert np.array(a['stats']).tobytes() == np.array(b['stats']).tobytes()
    for (ia, ba, sa, la), (ib, bb, sb, lb) in zip(a['evaluator']._preds, b['evaluator']._preds):
        assert ia == ib and (ba is None) == (bb is None)
        if ba is not None:
            assert torch.equal(ba, bb) and torch.equal(sa, sb) and torch.equal(la, lb)
    # max_samples cuts inside a planned batch
    loader = torch.utils.data.DataLoader(planned, batch_size=2, collate_fn=collate)
    assert E.evaluate_detection(model, loader, torch.device('cpu'), max_samples=1)['evaluator'].img_ids == [3]


def test_loader_workers_hand_planned_batches_over(S, tmp_path):
    planned, _ = _datasets(tmp_path, annotated_only=True, random_horizontal_flip=0.5)
    loader = torch.utils.data.DataLoader(planned, batch_size=2, num_workers=1, collate_fn=S.transforms.COLLATE_FUNC_DICT['coco_collate_fn'])
    (images, targets), = list(loader)
    assert isinstance(images, S.transforms.DeferredDetBatch) and images.sizes == [(36, 24), (30, 40)]
    assert [int(t['image_id']) for t in targets] == [3, 7]
