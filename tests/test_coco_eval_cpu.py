"""`CocoBoxEvaluator` on CPU tensors (the torch / numpy host path of sc2bench_amd/coco_eval.py) against the sequential restatement of
tests/ref_coco.py: precision, recall and the twelve statistics bit for bit; the three forms of ground truth, `coco_gt_from_dataset`,
the reference's attribute path, the printed lines, `evaluate_detection`, the `test_only` branch and a world-size-2 gloo group."""
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import coco_cases as C
from tests import ref_coco as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tensors(preds, device='cpu'):
    return {i: ({} if not p else {k: torch.from_numpy(v).to(device) for k, v in p.items()}) for i, p in preds.items()}


def run(S, gt, preds, batch=2):
    ev = S.CocoBoxEvaluator(gt)
    ids = list(preds)
    for i in range(0, len(ids), batch):      # several updates, in the order given
        ev.update({k: preds[k] for k in ids[i:i + batch]})
    ev.synchronize_between_processes()
    ev.accumulate()
    return ev


def same(ev, ref):
    be = ev.coco_eval['bbox']
    assert be.eval['precision'].shape == ref['precision'].shape and be.eval['recall'].shape == ref['recall'].shape
    assert np.array_equal(be.eval['precision'], ref['precision'])
    assert np.array_equal(be.eval['recall'], ref['recall'])
    ev.summarize()
    assert be.stats.dtype == np.float64 and be.stats.shape == (12,)
    assert be.stats.tobytes() == ref['stats'].tobytes()


@pytest.mark.parametrize('case', C.HAND_CASES, ids=lambda f: f.__name__)
def test_hand_cases_equal_the_restatement(S, case):
    gt, preds = case()
    ev = run(S, gt, tensors(preds))
    assert ev.coco_eval['bbox'].path == 'host'
    same(ev, R.evaluate(gt, preds))


@pytest.mark.parametrize('seed,kw', [(0, {}), (1, {}), (2, {'crowd': 0.5}), (3, {'empty': 0.6}), (4, {'images': 12, 'cats': (3, 4, 7, 9, 20)}),
                                     (5, {'images': 3, 'big_segment': 70}), (6, {'images': 2, 'max_det': 130, 'cats': (1,)})])
def test_random_sets_equal_the_restatement(S, seed, kw):
    gt, preds = C.random_case(seed, **kw)
    ref = R.evaluate(gt, preds)
    assert (ref['precision'] > 0).any()
    same(run(S, gt, tensors(preds), batch=3), ref)


def test_update_order_does_not_matter(S):
    gt, preds = C.random_case(7)
    t = tensors(preds)
    a = run(S, gt, t)
    b = run(S, gt, dict(reversed(list(t.items()))), batch=1)
    assert np.array_equal(a.coco_eval['bbox'].eval['precision'], b.coco_eval['bbox'].eval['precision'])
    assert a.img_ids != b.img_ids and sorted(a.img_ids) == sorted(b.img_ids)


def test_three_forms_of_ground_truth(S, tmp_path):
    gt, preds = C.random_case(8)
    ref = R.evaluate(gt, preds)
    path = tmp_path / 'instances.json'
    path.write_text(json.dumps(gt))

    class Index(object):      # what a pycocotools.COCO looks like from outside
        dataset = gt
    for form in (gt, str(path), path, Index()):
        same(run(S, form, tensors(preds)), ref)
    with pytest.raises(ValueError, match='COCO dictionary'):
        S.CocoBoxEvaluator([1, 2, 3])


def test_reference_attribute_path_and_printed_lines(S, capsys):
    gt, preds = C.tp_fp_tp()
    ref = R.evaluate(gt, preds)
    ev = run(S, gt, tensors(preds))
    capsys.readouterr()
    ev.summarize()
    printed = capsys.readouterr().out.splitlines()
    assert printed[0] == 'IoU metric: bbox' and printed[1:] == ref['lines'] and len(printed) == 13
    assert printed[1] == ' Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.835'
    val_iou_type = 'bbox'
    assert ev.coco_eval[val_iou_type].stats[0] == ref['stats'][0]      # object_detection.py:214


def test_other_iou_types_raise(S):
    gt, _ = C.perfect()
    with pytest.raises(ValueError, match='segm'):
        S.CocoBoxEvaluator(gt, iou_types=('bbox', 'segm'))
    with pytest.raises(ValueError, match='keypoints'):
        S.CocoBoxEvaluator(gt, iou_types=['keypoints'])
    assert S.CocoBoxEvaluator(gt, iou_types=['bbox']).iou_types == ('bbox',)


def test_update_keeps_device_tensors_untouched(S):
    """update only appends: the very tensor objects are buffered (no copy, no read)"""
    gt, preds = C.perfect()
    t = tensors(preds)
    ev = S.CocoBoxEvaluator(gt)
    ev.update(t)
    assert all(b is t[i]['boxes'] and s is t[i]['scores'] for i, b, s, _ in ev._preds)


class ToyDetection(torch.utils.data.Dataset):
    """(image, target) samples in torchvision's detection format, built from a COCO dictionary"""

    def __init__(self, gt):
        self.gt = gt
        self.ids = [im['id'] for im in gt['images']]

    def __len__(self):
        return len(self.ids)

    def __getitem__(self, index):
        image_id = self.ids[index]
        anns = [a for a in self.gt['annotations'] if a['image_id'] == image_id]
        boxes = torch.tensor([a['bbox'] for a in anns], dtype=torch.float32).reshape(-1, 4)
        boxes[:, 2:] += boxes[:, :2]
        target = {'boxes': boxes, 'labels': torch.tensor([a['category_id'] for a in anns], dtype=torch.int64),
                  'area': torch.tensor([a['area'] for a in anns], dtype=torch.float32),
                  'iscrowd': torch.tensor([a['iscrowd'] for a in anns], dtype=torch.int64), 'image_id': torch.tensor([image_id])}
        return torch.zeros(3, 24 + index, 32), target


def test_coco_gt_from_dataset(S):
    gt, preds = C.random_case(9, empty=0.0)
    data = ToyDetection(gt)
    got = S.coco_gt_from_dataset(data)
    assert [im['id'] for im in got['images']] == data.ids and got['images'][1] == {'id': data.ids[1], 'height': 25, 'width': 32}
    assert [a['id'] for a in got['annotations']] == list(range(1, len(gt['annotations']) + 1))
    assert [a['bbox'] for a in got['annotations']] == [a['bbox'] for a in gt['annotations']]      # (grid coordinates: exact in f32)
    assert [(a['image_id'], a['category_id'], a['area'], a['iscrowd']) for a in got['annotations']] == \
        [(a['image_id'], a['category_id'], a['area'], a['iscrowd']) for a in gt['annotations']]
    assert got['categories'] == [{'id': c} for c in sorted(set(a['category_id'] for a in gt['annotations']))]
    sub = torch.utils.data.Subset(torch.utils.data.Subset(data, [2, 0, 1]), [0, 1])
    assert [im['id'] for im in S.coco_gt_from_dataset(sub)['images']] == data.ids      # Subsets are unwrapped

    class Wrapped(ToyDetection):
        class coco(object):
            dataset = gt
    assert S.coco_gt_from_dataset(torch.utils.data.Subset(Wrapped(gt), [0])) is gt


def test_loader_over_a_coco_dictionary(S, tmp_path):
    """`--json '{"datasets": {<id>: {"coco_gt": ...}}}'`: the loader runs on the dictionary alone (noise images of the listed sizes)"""
    from sc2bench_amd import evaluation as E
    gt, _ = C.random_case(13, images=3, empty=0.0)
    path = tmp_path / 'toy.json'
    path.write_text(json.dumps(gt))
    for entry in ({'coco_gt': gt}, {'coco_gt': str(path), 'seed': 4}):
        loader = E.build_data_loader({'val': entry}, {'dataset_id': 'val', 'collate_fn': 'coco_collate_fn', 'kwargs': {'batch_size': 2}})
        assert isinstance(loader.dataset, S.CocoDictDetection) and S.coco_gt_from_dataset(loader.dataset) == gt
        images, targets = next(iter(loader))
        assert len(images) == 2 and images[0].shape == (3, 512, 512) and images[0].dtype == torch.float32
        anns = [a for a in gt['annotations'] if a['image_id'] == gt['images'][0]['id']]
        assert int(targets[0]['image_id']) == gt['images'][0]['id'] and targets[0]['labels'].tolist() == [a['category_id'] for a in anns]
        b = targets[0]['boxes'][0].tolist()
        assert [b[0], b[1], b[2] - b[0], b[3] - b[1]] == anns[0]['bbox'] and targets[0]['iscrowd'].dtype == torch.int64


class CannedDetector(torch.nn.Module):
    """Returns stored detections by the image's height (ToyDetection gives every image its own)."""

    def __init__(self, by_height):
        super().__init__()
        self.by_height = by_height
        self.calls = 0

    def forward(self, images):
        self.calls += 1
        assert isinstance(images, list) and not self.training
        return [self.by_height[int(im.shape[-2])] for im in images]


def canned(gt, preds):
    data = ToyDetection(gt)
    t = tensors(preds)
    empty = {'boxes': torch.zeros(0, 4), 'scores': torch.zeros(0), 'labels': torch.zeros(0, dtype=torch.int64)}
    return data, CannedDetector({24 + i: (t[image_id] or empty) for i, image_id in enumerate(data.ids)})


def test_evaluate_detection_on_a_stub_model(S):
    from sc2bench_amd import evaluation as E
    gt, preds = C.random_case(10, images=5)
    ref = R.evaluate(gt, preds)
    data, model = canned(gt, preds)
    loader = torch.utils.data.DataLoader(data, batch_size=2, collate_fn=S.transforms.COLLATE_FUNC_DICT['coco_collate_fn'])
    res = E.evaluate_detection(model, loader, torch.device('cpu'), gt=gt)
    assert set(res) >= {'map', 'stats', 'samples', 'seconds', 'analysis', 'evaluator'}
    assert res['samples'] == 5 and model.calls == 3 and res['map'] == ref['stats'][0]
    assert np.array(res['stats']).tobytes() == ref['stats'].tobytes()
    assert res['evaluator'].coco_eval['bbox'].stats[0] == ref['stats'][0]
    # gt=None: the dictionary is rebuilt from the dataset; max_samples stops inside a batch
    sub = {i: preds[i] for i in data.ids[:3]}
    res3 = E.evaluate_detection(model, loader, torch.device('cpu'), max_samples=3)
    gt3 = S.coco_gt_from_dataset(data)
    assert res3['samples'] == 3 and np.array(res3['stats']).tobytes() == R.evaluate(gt3, sub)['stats'].tobytes()


def test_test_only_sends_a_faster_rcnn_to_evaluate_detection(S, monkeypatch, capsys):
    from sc2bench_amd import evaluation as E
    gt, preds = C.random_case(11, images=4, empty=0.0)
    data, stub = canned(gt, preds)

    class Detector(S.detection.FasterRCNN):      # a FasterRCNN by type, the stub's outputs
        def __init__(self):
            torch.nn.Module.__init__(self)

        def forward(self, images, targets=None):
            return stub.eval()(images)
    monkeypatch.setattr(E.C, 'build_model', lambda model_config, device: Detector())
    config = {'models': {'model': {'key': 'stub', 'kwargs': {}}}, 'datasets': {'val': data},
              'test': {'test_data_loader': {'dataset_id': 'val', 'kwargs': {'batch_size': 2}, 'collate_fn': 'coco_collate_fn'}}}
    res = E.test_only(config, torch.device('cpu'))
    ref = R.evaluate(S.coco_gt_from_dataset(data), preds)
    assert res['samples'] == 4 and np.array(res['stats']).tobytes() == ref['stats'].tobytes()
    assert res['summary'].splitlines()[1:] == ref['lines']


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _world2_worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ.update({'MASTER_ADDR': '127.0.0.1', 'MASTER_PORT': str(port), 'RANK': str(rank), 'WORLD_SIZE': str(world),
                       'LOCAL_RANK': str(rank), 'HIP_VISIBLE_DEVICES': '-1', 'CUDA_VISIBLE_DEVICES': '-1'})
    import sc2bench_amd as S
    from sc2bench_amd import dataparallel as dp
    dp.init_distributed(backend='gloo')
    gt, preds = C.random_case(12, images=7)
    t = tensors(preds)
    ids = list(t)
    # rank 0: images 0..3, rank 1: images 3..6 -- image 3 on both, rank 1's copy with other boxes: rank 0's must win
    mine = {i: t[i] for i in (ids[:4] if rank == 0 else ids[3:])}
    if rank == 1:
        mine[ids[3]] = {'boxes': torch.tensor([[0., 0., 64., 64.]]), 'scores': torch.tensor([1.0]), 'labels': torch.tensor([1])}
    ev = S.CocoBoxEvaluator(gt)
    ev.update(mine)
    ev.synchronize_between_processes()
    ev.accumulate()
    ev.summarize()
    be = ev.coco_eval['bbox']
    out[rank] = (be.eval['precision'].tobytes(), be.eval['recall'].tobytes(), be.stats.tobytes(), sorted(ev.img_ids))
    dist.barrier()
    dist.destroy_process_group()


def test_world2_split_and_duplicated_images_equal_one_process(S):
    world, port = 2, _free_port()
    ctx = mp.get_context('spawn')
    with ctx.Manager() as mgr:
        out = mgr.dict()
        procs = [ctx.Process(target=_world2_worker, args=(r, world, port, out)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=240)
            assert p.exitcode == 0
        res = dict(out)
    gt, preds = C.random_case(12, images=7)
    ref = R.evaluate(gt, preds)
    for r in range(world):
        assert res[r][0] == ref['precision'].tobytes() and res[r][1] == ref['recall'].tobytes() and res[r][2] == ref['stats'].tobytes()
        assert res[r][3] == sorted(preds)
