"""sc2_coco_match / sc2_coco_accumulate on the device against the sequential restatement of tests/ref_coco.py -- flags, npig, precision
and recall bit for bit, no tolerance -- and `CocoBoxEvaluator` on device tensors against the same evaluator on CPU tensors."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests import coco_cases as C
from tests import ref_coco as R

pytestmark = pytest.mark.gpu

TILE_D, TILE_G, CHUNK = 100, 64, 1024      # SC2_COCO_TILE_DETS, SC2_COCO_TILE_GTS, SC2_COCO_SCAN_CHUNK
POISON = 0x5A5A5A5A
# detections x ground truths of the first segments: empty ones, one pair, a full detection tile, one ground truth more than the tile
# holds (the workspace path), exactly the tile, both counts beyond the tile
SHAPES = [(0, 0), (0, 3), (3, 0), (1, 1), (TILE_D, 1), (64, TILE_G + 1), (7, TILE_G), (TILE_D + 30, TILE_G + 6)]


def _segment(rng, D, G):
    """dets [D,4] and gts [G,4] xywh on an 8-pixel lattice (duplicates, nested halves: IoU exactly 0.5, 0.75 ...), `area` fields partly
    out of range, crowds"""
    g = C.random_boxes(rng, G, side=10)
    d = C.random_boxes(rng, D, side=10)
    for i in range(min(D, G)):      # a third of the detections copy a ground truth, a sixth cover exactly half of one
        u = rng.rand()
        if u < 0.33:
            d[i] = g[rng.randint(G)]
        elif u < 0.5:
            d[i] = g[rng.randint(G)] * np.array([1, 1, 1, 0.5])
    area = g[:, 2] * g[:, 3] * rng.choice([1.0, 1.0, 1.0, 0.25, 8.0, 40.0], size=G)
    crowd = (rng.rand(G) < 0.2).astype(np.uint8)
    return d, g, area, crowd


@pytest.fixture(scope='module')
def match_case():
    """several hundred mixed segments and the restatement's answer, computed once"""
    rng = np.random.RandomState(5)
    shapes = SHAPES + [(int(rng.randint(0, 9)), int(rng.randint(0, 7))) for _ in range(300)]
    segs = [_segment(rng, D, G) for D, G in shapes]
    want_flags, want_npig = [], []
    for d, g, area, crowd in segs:
        matched, ignored, npig, _ = R.match_segment(d.tolist(), g.tolist(), area.tolist(), crowd.tolist())
        want_flags += [R.flag_words(matched, ignored, i) for i in range(len(d))]
        want_npig.append(npig)
    return {'dets': np.concatenate([s[0] for s in segs]), 'gts': np.concatenate([s[1] for s in segs]),
            'area': np.concatenate([s[2] for s in segs]), 'crowd': np.concatenate([s[3] for s in segs]),
            'det_off': np.cumsum([0] + [s[0] for s in shapes]).astype(np.int32), 'gt_off': np.cumsum([0] + [s[1] for s in shapes]).astype(np.int32),
            'flags': np.array(want_flags, dtype=np.int32).reshape(-1, 4), 'npig': np.array(want_npig, dtype=np.int32).reshape(-1, 4)}


def _match(S, dev, c, lo=0, hi=None):
    """segments lo..hi-1 of the case in one launch, outputs pre-filled with a poison pattern"""
    hi = len(c['det_off']) - 1 if hi is None else hi
    d0, d1, g0, g1 = c['det_off'][lo], c['det_off'][hi], c['gt_off'][lo], c['gt_off'][hi]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    flags = torch.full((int(d1 - d0), 4), POISON, dtype=torch.int32, device=dev)
    npig = torch.full((hi - lo, 4), POISON, dtype=torch.int32, device=dev)
    out = S.hip.coco_match(t(c['dets'][d0:d1]), t(c['gts'][g0:g1]), t(c['area'][g0:g1]), t(c['crowd'][g0:g1]), t(c['det_off'][lo:hi + 1] - d0),
                           t(c['gt_off'][lo:hi + 1] - g0), t(R.IOU_THRS), t(np.array(R.AREA_RNG)), flags=flags, npig=npig)
    assert out[0] is flags and out[1] is npig
    return flags.cpu().numpy(), npig.cpu().numpy(), (d0, d1)


@pytest.mark.parametrize('seg', range(len(SHAPES)), ids=['{}x{}'.format(*s) for s in SHAPES])
def test_match_one_segment(S, dev, match_case, seg):
    flags, npig, (d0, d1) = _match(S, dev, match_case, seg, seg + 1)
    assert np.array_equal(npig, match_case['npig'][seg:seg + 1])
    assert np.array_equal(flags, match_case['flags'][d0:d1])


def test_match_all_segments_in_one_launch(S, dev, match_case):
    flags, npig, _ = _match(S, dev, match_case)
    assert len(npig) > 300 and not (flags == POISON).any() and not (npig == POISON).any()
    assert np.array_equal(npig, match_case['npig'])
    assert np.array_equal(flags, match_case['flags'])
    again = _match(S, dev, match_case)
    assert np.array_equal(again[0], flags) and np.array_equal(again[1], npig)


def test_match_zero_segments_and_bad_arguments(S, dev):
    z = lambda *shape, dtype=torch.float64: torch.zeros(*shape, dtype=dtype, device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    thr, rng = t(R.IOU_THRS), t(np.array(R.AREA_RNG))
    flags, npig = S.hip.coco_match(z(0, 4), z(0, 4), z(0), z(0, dtype=torch.uint8), z(1, dtype=torch.int32), z(1, dtype=torch.int32), thr, rng)
    assert flags.shape == (0, 4) and npig.shape == (0, 4)
    with pytest.raises(ValueError):
        S.hip.coco_match(z(2, 4, dtype=torch.float32), z(0, 4), z(0), z(0, dtype=torch.uint8), z(2, dtype=torch.int32), z(2, dtype=torch.int32), thr, rng)
    with pytest.raises(S.hip.Sc2Error):
        S.hip.coco_match(torch.zeros(0, 4, dtype=torch.float64), z(0, 4), z(0), z(0, dtype=torch.uint8), z(1, dtype=torch.int32),
                         z(1, dtype=torch.int32), thr, rng)


# ------------------------------------------------------------------------------------------------------------ accumulate
CAT_SIZES = [0, 1, CHUNK, CHUNK + 1, 3 * CHUNK + 77, 40, 0]      # detections per category; the last two: npig = 0


@pytest.fixture(scope='module')
def acc_case():
    rng = np.random.RandomState(11)
    n = sum(CAT_SIZES)
    bits = rng.randint(0, 1 << 10, size=(n, 4))
    ign = rng.randint(0, 1 << 10, size=(n, 4)) & rng.randint(0, 1 << 10, size=(n, 4))      # a quarter of the bits
    flags = (bits | (ign << 10)).astype(np.int32)
    rank = rng.choice([0, 0, 0, 1, 2, 5, 9, 10, 11, 50, 99, 100, 120], size=n).astype(np.int32)
    place = rng.permutation(n).astype(np.int32)      # the order array walks the flags in a scattered order
    cat_off = np.cumsum([0] + CAT_SIZES).astype(np.int32)
    npig = rng.randint(1, 400, size=(len(CAT_SIZES), 4)).astype(np.int32)
    npig[-2:] = 0
    npig[2, 1] = 0
    K = len(CAT_SIZES)
    precision, recall = -np.ones((10, 101, K, 4, 3)), -np.ones((10, K, 4, 3))
    for k in range(K):
        idx = place[cat_off[k]:cat_off[k + 1]]
        for a in range(4):
            for mi, max_det in enumerate(R.MAX_DETS):
                entries = [([(flags[o, a] >> t) & 1 for t in range(10)], [(flags[o, a] >> (10 + t)) & 1 for t in range(10)])
                           for o in idx if rank[o] < max_det]
                got = R.curves(entries, int(npig[k, a]))
                if got is not None:
                    precision[:, :, k, a, mi], recall[:, k, a, mi] = np.array(got[0]), np.array(got[1])
    return {'order': place, 'cat_off': cat_off, 'flags': flags, 'rank': rank, 'npig': npig, 'precision': precision, 'recall': recall}


def test_accumulate_equals_the_restatement(S, dev, acc_case):
    c = acc_case
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = (t(c['order']), t(c['cat_off']), t(c['flags']), t(c['rank']), t(c['npig']), t(R.REC_THRS), t(np.array(R.MAX_DETS, dtype=np.int32)))
    precision, recall = S.hip.coco_accumulate(*args)
    assert precision.shape == c['precision'].shape and recall.shape == c['recall'].shape
    assert (c['precision'][:, :, 4] > 0).any() and (c['recall'][:, 1] > 0).any()
    assert np.array_equal(recall.cpu().numpy(), c['recall'])
    assert np.array_equal(precision.cpu().numpy(), c['precision'])
    again = S.hip.coco_accumulate(*args)
    assert torch.equal(again[0], precision) and torch.equal(again[1], recall)
    # no categories: nothing is launched
    p0, r0 = S.hip.coco_accumulate(args[0][:0], args[1][:1], args[2], args[3], args[4][:0], args[5], args[6])
    assert p0.shape == (10, 101, 0, 4, 3) and r0.shape == (10, 0, 4, 3)


# ------------------------------------------------------------------------------------------------------------ the evaluator
def _tensors(preds, device):
    return {i: ({} if not p else {k: torch.from_numpy(v).to(device) for k, v in p.items()}) for i, p in preds.items()}


def _evaluate(S, gt, preds):
    ev = S.CocoBoxEvaluator(gt)
    ev.update(preds)
    ev.synchronize_between_processes()
    ev.accumulate()
    ev.summarize()
    return ev.coco_eval['bbox']


@pytest.mark.parametrize('seed,kw', [(0, {}), (2, {'crowd': 0.5}), (3, {'empty': 0.6}), (5, {'images': 3, 'big_segment': 70}),
                                     (6, {'images': 2, 'max_det': 130, 'cats': (1,)})])
def test_evaluator_on_device_tensors_equals_cpu_tensors(S, dev, seed, kw):
    gt, preds = C.random_case(seed, **kw)
    on_dev = _evaluate(S, gt, _tensors(preds, dev))
    on_cpu = _evaluate(S, gt, _tensors(preds, 'cpu'))
    ref = R.evaluate(gt, preds)
    assert on_dev.path == 'hip' and on_cpu.path == 'host'
    for got in (on_dev, on_cpu):
        assert np.array_equal(got.eval['precision'], ref['precision']) and np.array_equal(got.eval['recall'], ref['recall'])
        assert got.stats.tobytes() == ref['stats'].tobytes()


def test_switch_off_takes_the_host_path(S, dev, monkeypatch):
    gt, preds = C.tp_fp_tp()
    monkeypatch.setattr(S.hip.host_policy, 'coco_eval_hip', False)
    got = _evaluate(S, gt, _tensors(preds, dev))
    assert got.path == 'host' and got.stats.tobytes() == R.evaluate(gt, preds)['stats'].tobytes()


def test_detections_of_a_faster_rcnn(S, dev):
    """the real output types: detections straight from `detection.FasterRCNN` (random weights, fixed random pyramid features, one
    160 x 208 image) into `update`; ground truth = some of its own boxes, so that matches exist"""
    from sc2bench_amd import detection

    class Pyramid(torch.nn.Module):
        out_channels = 256

        def forward(self, x):
            g = torch.Generator().manual_seed(19)
            H, W = x.shape[-2:]
            return OrderedDict((name, torch.randn(x.shape[0], 256, -(-H // s), -(-W // s), generator=g).to(x.device))
                               for name, s in zip(['1', '2', '3', '4', 'pool'], [4, 8, 16, 32, 64]))
    torch.manual_seed(19)
    model = detection.FasterRCNN(Pyramid(), 5, min_size=160, max_size=208, rpn_post_nms_top_n_test=100, box_score_thresh=0.0).eval()
    with torch.no_grad():
        model.roi_heads.box_predictor.bbox_pred.weight.mul_(8.0)
        model.roi_heads.box_predictor.cls_score.weight.mul_(8.0)
        out = model.to(dev)([torch.rand(3, 160, 208, generator=torch.Generator().manual_seed(0)).to(dev)])
    assert len(out) == 1 and out[0]['boxes'].is_cuda and 0 < out[0]['boxes'].shape[0] <= 100
    host = {k: v.cpu() for k, v in out[0].items()}
    anns = []
    for j in range(0, host['boxes'].shape[0], 3):
        x1, y1, x2, y2 = host['boxes'][j].double().tolist()
        anns.append(C.ann(7, int(host['labels'][j]), x1, y1, x2 - x1 + 1.0, y2 - y1, crowd=int(j % 12 == 0)))
    gt = C.gt_dict(anns, cats=(1, 2, 3, 4))
    on_dev = _evaluate(S, gt, {7: out[0]})
    on_cpu = _evaluate(S, gt, {7: host})
    ref = R.evaluate(gt, {7: {k: v.numpy() for k, v in host.items()}})
    assert on_dev.path == 'hip' and (ref['precision'] > 0).any()
    assert np.array_equal(on_dev.eval['precision'], ref['precision']) and np.array_equal(on_dev.eval['recall'], ref['recall'])
    assert on_dev.stats.tobytes() == ref['stats'].tobytes() == on_cpu.stats.tobytes()
