"""GPU: the detection kernels (csrc/detect.hip) against tests/ref_detection.py, the RPN + RoI heads on them against the same
modules on torch ops, and the whole Faster R-CNN once."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_detection as RD  # noqa: E402

pytestmark = pytest.mark.gpu

_NMS_CASES = RD.nms_cases()


# ------------------------------------------------------------------------------------------------------------------ NMS
@pytest.mark.parametrize('case', _NMS_CASES, ids=[c[0] for c in _NMS_CASES])
def test_nms_equals_sequential_reference(S, dev, case):
    """kept indices, their order and the count equal the float32 sequential reference exactly; `keep` sits inside a larger
    buffer of sentinels: every byte outside it is untouched, every byte inside is written (0 or 1)"""
    from sc2bench_amd import detection
    _, boxes, scores, groups, thr = case
    n = boxes.shape[0]
    want = RD.batched_nms_ref(boxes, scores, groups, thr)
    tb, ts, tg = torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), torch.from_numpy(groups).to(dev)
    got = detection.batched_nms(tb, ts, tg, thr)
    assert got.dtype == torch.int64 and got.tolist() == want.tolist()
    # the entry point itself, writing into the middle of a guarded buffer
    order = torch.sort(ts, descending=True, stable=True)[1]
    guard = torch.full((n + 256,), 0xAB, dtype=torch.uint8, device=dev)
    keep, count = S.hip.nms_sorted(tb[order].contiguous(), tg[order].to(torch.int32).contiguous(), thr, keep=guard[128:128 + n])
    torch.cuda.synchronize()
    host = guard.cpu().numpy()
    assert np.all(host[:128] == 0xAB) and np.all(host[128 + n:] == 0xAB), 'nms wrote outside keep'
    inside = host[128:128 + n]
    assert np.all(inside <= 1), 'nms left a byte of keep unwritten'
    assert order.cpu().numpy()[inside.astype(bool)].tolist() == want.tolist()
    assert int(count.item()) == len(want)


def test_nms_empty_and_over_the_cap(S, dev):
    from sc2bench_amd import detection
    empty = detection.batched_nms(torch.zeros((0, 4), device=dev), torch.zeros(0, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), 0.5)
    assert empty.dtype == torch.int64 and empty.numel() == 0
    keep, count = S.hip.nms_sorted(torch.zeros((0, 4), device=dev), torch.zeros(0, dtype=torch.int32, device=dev), 0.5)
    assert keep.numel() == 0 and int(count.item()) == 0
    assert S.hip.lib().sc2_nms_ws_bytes(S.hip.NMS_MAX_BOXES) == 32 << 20 and S.hip.lib().sc2_nms_ws_bytes(S.hip.NMS_MAX_BOXES + 1) == 0
    # 20 000 boxes in 4 groups: split by group into several calls, the result is that of one
    boxes, scores, groups = RD.random_boxes(20000, 4, seed=20000, extent=1500.0)
    want = RD.batched_nms_ref(boxes, scores, groups, 0.5)
    got = detection.batched_nms(torch.from_numpy(boxes).to(dev), torch.from_numpy(scores).to(dev), torch.from_numpy(groups).to(dev), 0.5)
    assert got.tolist() == want.tolist()
    # a single group above the cap cannot be split
    n = S.hip.NMS_MAX_BOXES + 1
    with pytest.raises(ValueError, match='single group'):
        detection.batched_nms(torch.from_numpy(boxes[:n]).to(dev), torch.from_numpy(scores[:n]).to(dev),
                              torch.zeros(n, dtype=torch.int64, device=dev), 0.5)
    with pytest.raises(ValueError):
        S.hip.nms_sorted(torch.zeros((n, 4), device=dev), torch.zeros(n, dtype=torch.int32, device=dev), 0.5)


# ------------------------------------------------------------------------------------------------------------ RoIAlign
def _roi_run(S, dev, C, P, K, seed, bf16, mode):
    feats = RD.roi_features(C, seed=C)
    tf = [torch.from_numpy(f).to(dev) for f in feats]
    if bf16:
        tf = [f.to(torch.bfloat16) for f in tf]
        feats = [f.float().cpu().numpy() for f in tf]        # the reference sees the rounded inputs
    rois, levels, dropped = RD.roi_cases(K, seed, P, 2, mode)
    assert dropped <= 0.05 * K, '{} of {} RoIs fell into the exclusion band: pick another seed'.format(dropped, K)
    want = RD.roi_align_ref(feats, RD.SCALES, rois, levels, P, 2)
    nhwc = [f.permute(0, 2, 3, 1).contiguous() for f in tf]
    total = K * C * P * P
    guard = torch.full((total + 2048,), float('nan'), dtype=torch.float32, device=dev)
    out = guard[1024:1024 + total].view(K, C, P, P)
    got = S.hip.roi_align(nhwc, RD.SCALES, torch.from_numpy(rois).to(dev), torch.from_numpy(levels).to(torch.int32).to(dev), P, 2, out=out)
    torch.cuda.synchronize()
    host = guard.cpu().numpy()
    assert np.all(np.isnan(host[:1024])) and np.all(np.isnan(host[1024 + total:])), 'roi_align wrote outside its output'
    assert not np.any(np.isnan(host[1024:1024 + total])), 'roi_align left an output element unwritten'
    assert got.data_ptr() == out.data_ptr()
    err = np.abs(host[1024:1024 + total].reshape(K, C, P, P).astype(np.float64) - want).max()
    scale = max(np.abs(f).max() for f in feats)
    print('roi_align C={} P={} K={} {} {}: max |err| = {:.3e} = 2^{:.1f} * max|x|'.format(
        C, P, K, 'bf16' if bf16 else 'f32', mode, err, np.log2(max(err, 1e-300) / scale)))
    return err, scale, (tf, rois, levels)


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('K,seed', [(1, 11), (37, 12), (300, 13)])
@pytest.mark.parametrize('P', [7, 2])
@pytest.mark.parametrize('C', [8, 256])
def test_roi_align_equals_reference(S, dev, C, P, K, seed, bf16):
    """|err| <= 2^-12 * max|x| against the float64 reference on the same f32- / bf16-rounded inputs: some six f32 roundings per
    coordinate at magnitude < 64 move a sample by <= 2^-15.4 px, the bilinear slope is <= 2 * max|x| per axis, two axes give
    2^-13.4, and 2^-12 leaves x 1.5 over that plus the summation error.  RoIs with a float64 sample within 2^-10 of -1 or of
    H / W (where the definition jumps) are left out by the generator, at most 5 % of them.
    Observed on an MI355X, maximum over these cases (C = 256, P = 7, K = 300): the kernel 1.38e-5 = 2^-18.4 * max|x|, an f32
    torch-op restatement on the same device 1.38e-5 = 2^-18.4 * max|x| (test_roi_align_torch_op_restatement_on_the_device)."""
    from sc2bench_amd import detection
    err, scale, (tf, rois, levels) = _roi_run(S, dev, C, P, K, seed, bf16, 'mixed')
    assert err <= 2.0 ** -12 * scale
    # the package's dispatch reaches the same kernel from NCHW maps
    got = detection.multiscale_roi_align(tf, RD.SCALES, torch.from_numpy(rois).to(dev), torch.from_numpy(levels).to(dev), P, 2)
    direct = S.hip.roi_align([f.permute(0, 2, 3, 1).contiguous() for f in tf], RD.SCALES, torch.from_numpy(rois).to(dev),
                             torch.from_numpy(levels).to(torch.int32).to(dev), P, 2)
    assert torch.equal(got, direct)


@pytest.mark.parametrize('mode', ['one', 'skip'])
@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
def test_roi_align_one_level_and_an_unused_level(S, dev, mode, bf16):
    """all RoIs on one map; a map no RoI is pooled from"""
    err, scale, _ = _roi_run(S, dev, 256, 7, 37, 12, bf16, mode)
    assert err <= 2.0 ** -12 * scale


def test_roi_align_torch_op_restatement_on_the_device(S, dev, monkeypatch):
    """the f32 torch-op restatement (the A/B path) against the same reference and bound, and its distance from the kernel"""
    from sc2bench_amd import detection
    feats = RD.roi_features(256, seed=256)
    tf = [torch.from_numpy(f).to(dev) for f in feats]
    rois, levels, _ = RD.roi_cases(300, 13, 7, 2, 'mixed')
    want = RD.roi_align_ref(feats, RD.SCALES, rois, levels, 7, 2)
    args = (tf, RD.SCALES, torch.from_numpy(rois).to(dev), torch.from_numpy(levels).to(dev), 7, 2)
    kernel = detection.multiscale_roi_align(*args)
    monkeypatch.setattr(S.hip.host_policy, 'roi_align_hip', False)
    torch_op = detection.multiscale_roi_align(*args)
    scale = max(np.abs(f).max() for f in feats)
    e_t = np.abs(torch_op.cpu().numpy().astype(np.float64) - want).max()
    e_k = np.abs(kernel.cpu().numpy().astype(np.float64) - want).max()
    print('torch-op restatement: max |err| = {:.3e} (2^{:.1f} * max|x|); kernel {:.3e} (2^{:.1f}); between them {:.3e}'.format(
        e_t, np.log2(e_t / scale), e_k, np.log2(e_k / scale), (kernel - torch_op).abs().max().item()))
    assert e_t <= 2.0 ** -12 * scale and e_k <= 2.0 ** -12 * scale


def test_roi_align_rejects_what_it_cannot_read(S, dev):
    f = torch.zeros(1, 4, 4, 8, device=dev)
    rois, lv = torch.zeros(1, 5, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        S.hip.roi_align([f], [1.0], rois, lv, 15, 2)
    with pytest.raises(ValueError):
        S.hip.roi_align([f], [1.0], rois, lv, 7, 0)
    with pytest.raises(ValueError):
        S.hip.roi_align([torch.zeros(1, 4, 4, 12, device=dev)], [1.0], rois, lv, 7, 2)
    # a level or an image that does not exist reads nothing and comes back NaN
    bad = torch.tensor([[0.0, 0, 0, 2, 2], [3.0, 0, 0, 2, 2], [0.0, 0, 0, 2, 2]], device=dev)
    out = S.hip.roi_align([f + 1.0], [1.0], bad, torch.tensor([0, 0, 2], dtype=torch.int32, device=dev), 2, 2)
    assert torch.all(out[0] == 1.0) and torch.all(torch.isnan(out[1])) and torch.all(torch.isnan(out[2]))


# ------------------------------------------------------------------------------------------------------------ the tail
TAIL_SEED = 19      # of seeds 1..119 the one with the widest margin of the precondition below on the CPU: 1.8e-3
TAIL_IMAGE = (160, 208)
TAIL_CLASSES = 5


def tail_modules(device, seed=TAIL_SEED):
    """RPN + RoI heads with seeded random weights, fixed random f32 pyramid features (2 images, the configs' names)"""
    from sc2bench_amd import detection

    class Pyramid(torch.nn.Module):
        out_channels = 256
    torch.manual_seed(seed)
    model = detection.FasterRCNN(Pyramid(), TAIL_CLASSES, min_size=TAIL_IMAGE[0], max_size=TAIL_IMAGE[1], rpn_post_nms_top_n_test=100,
                                 box_score_thresh=0.0).eval()
    with torch.no_grad():       # regression outputs large enough to move boxes, logits spread enough to rank
        model.roi_heads.box_predictor.bbox_pred.weight.mul_(8.0)
        model.roi_heads.box_predictor.cls_score.weight.mul_(8.0)
    g = torch.Generator().manual_seed(seed)
    H, W = TAIL_IMAGE
    feats = OrderedDict((name, torch.randn(2, 256, -(-H // s), -(-W // s), generator=g))
                        for name, s in zip(['1', '2', '3', '4', 'pool'], [4, 8, 16, 32, 64]))
    images = detection.ImageList(torch.zeros(2, 3, H, W), [(H, W), (H - 12, W - 20)])
    return model.to(device), OrderedDict((k, v.to(device)) for k, v in feats.items()), images.to(device)


class _Computed(torch.nn.Module):
    """stands in for the RPN head: returns what the head computed once"""

    def __init__(self, out):
        super().__init__()
        self.out = out

    def forward(self, x):
        return self.out


def tail_run(model, feats, images, monkeypatch):
    """-> (proposals, detections, the final NMS calls' inputs)"""
    from sc2bench_amd import detection
    calls = []
    real = detection.batched_nms

    def recording(boxes, scores, idxs, thr):
        calls.append((boxes.detach().cpu().double().numpy(), scores.detach().cpu().numpy(), idxs.detach().cpu().numpy(), thr))
        return real(boxes, scores, idxs, thr)
    monkeypatch.setattr(detection, 'batched_nms', recording)
    with torch.no_grad():
        proposals, _ = model.rpn(images, feats)
        detections, _ = model.roi_heads(feats, proposals, images.image_sizes)
    monkeypatch.setattr(detection, 'batched_nms', real)
    return proposals, detections, [c for c in calls if c[3] == model.roi_heads.nms_thresh]


def closest_compared_pair(calls):
    """over the final NMS calls: min |IoU - threshold| over the pairs that decide (an earlier KEPT box against a later box of its
    label), IoU in float64"""
    closest = np.inf
    for boxes, scores, labels, thr in calls:
        order = np.argsort(-scores.astype(np.float64), kind='stable')
        b, g = boxes[order], labels[order]
        keep = RD.nms_ref(b, g, thr)
        area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        for j in np.nonzero(keep)[0]:
            later = slice(j + 1, None)
            w = np.maximum(0, np.minimum(b[j, 2], b[later, 2]) - np.maximum(b[j, 0], b[later, 0]))
            h = np.maximum(0, np.minimum(b[j, 3], b[later, 3]) - np.maximum(b[j, 1], b[later, 1]))
            iou = w * h / (area[j] + area[later] - w * h)
            d = np.abs(iou - thr)[g[later] == g[j]]
            if d.size:
                closest = min(closest, d.min())
    return closest


def test_tail_on_kernels_equals_tail_on_torch_ops(S, dev, monkeypatch):
    """RPN + RoI heads on the kernels against the same modules with both switches off, on the same device and features:
    proposals bit-identical, detections with the same count and labels, boxes within 1e-3 px, scores within 1e-5.
    Precondition (asserted): in the switches-off run no pair the final NMS decides on lies within 1e-3 of its threshold.
    The RPN head's convolutions are torch ops whose results are not bit-reproducible from call to call on the device (measured:
    two calls on the same features differ by 4.5e-8), so the head runs once and both runs start from its outputs."""
    model, feats, images = tail_modules(dev)
    with torch.no_grad():
        model.rpn.head = _Computed(model.rpn.head(list(feats.values())))
    prop_k, det_k, _ = tail_run(model, feats, images, monkeypatch)
    monkeypatch.setattr(S.hip.host_policy, 'nms_hip', False)
    monkeypatch.setattr(S.hip.host_policy, 'roi_align_hip', False)
    prop_t, det_t, final_calls = tail_run(model, feats, images, monkeypatch)
    assert len(final_calls) == 2
    margin = closest_compared_pair(final_calls)
    assert margin > 1e-3, 'seed {}: a decided pair of the final NMS lies {:.2e} from the threshold; pick another seed'.format(TAIL_SEED, margin)
    assert len(prop_k) == len(prop_t) == 2
    for a, b in zip(prop_k, prop_t):
        assert 0 < a.shape[0] <= 100 and torch.equal(a, b), 'proposals differ'
    for a, b in zip(det_k, det_t):
        assert 0 < a['boxes'].shape[0] <= 100
        assert a['boxes'].shape == b['boxes'].shape and torch.equal(a['labels'], b['labels'])
        assert (a['boxes'] - b['boxes']).abs().max().item() <= 1e-3
        assert (a['scores'] - b['scores']).abs().max().item() <= 1e-5


def test_faster_rcnn_end_to_end(S, dev):
    """the full `faster_rcnn_model` (bf16 HIP backbone + pyramid, RPN, RoI heads on the kernels) on one 320 x 416 image"""
    from sc2bench_amd import dense
    from test_detection_cpu import BACKBONE_CONFIG, MODEL_KWARGS
    torch.manual_seed(0)
    model = dense.faster_rcnn_model(BACKBONE_CONFIG, min_size=320, max_size=416, box_score_thresh=0.0, **MODEL_KWARGS)
    model.eval().to(dev)
    model.update()
    model.backbone.body.set_compute_dtype('bf16')
    model.backbone.fpn.to(torch.bfloat16)
    x = torch.rand(1, 3, 320, 416, generator=torch.Generator().manual_seed(0)).to(dev)
    with torch.no_grad():
        out = model([x[0]])
    torch.cuda.synchronize()
    assert len(out) == 1
    boxes, labels, scores = out[0]['boxes'], out[0]['labels'], out[0]['scores']
    d = boxes.shape[0]
    assert 0 < d <= 100 and boxes.shape == (d, 4) and boxes.dtype == torch.float32 and labels.dtype == torch.int64
    assert torch.isfinite(boxes).all() and torch.isfinite(scores).all()
    assert labels.min() >= 1 and labels.max() <= 90 and torch.all(scores[:-1] >= scores[1:])
    assert boxes[:, 0::2].min() >= 0 and boxes[:, 0::2].max() <= 416 and boxes[:, 1::2].min() >= 0 and boxes[:, 1::2].max() <= 320
