"""CPU: the detection tail (sc2-benchmark_amd/detection.py) -- `faster_rcnn_model` without torchvision, parameter names, anchors,
transform arithmetic, the torch-op NMS / RoIAlign against tests/ref_detection.py, one eval forward, the pooler's name filter."""
import os
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_detection as RD  # noqa: E402

# the student model of configs/coco2017/supervised_compression/entropic_student/faster_rcnn_splittable_resnet50-fp-beta*.yaml
BACKBONE_CONFIG = {'key': 'splittable_resnet',
                   'kwargs': {'num_classes': 1000, 'pretrained': True,
                              'bottleneck_config': {'key': 'FPBasedResNetBottleneck',
                                                    'kwargs': {'num_bottleneck_channels': 24, 'num_target_channels': 256}},
                              'resnet_name': 'resnet50', 'pre_transform': None, 'skips_avgpool': True, 'skips_fc': True}}
RETURN_LAYERS = {'bottleneck_layer': '1', 'layer2': '2', 'layer3': '3', 'layer4': '4'}
MODEL_KWARGS = dict(pretrained=True, pretrained_backbone_name='resnet50', progress=True, num_classes=91,
                    backbone_fpn_kwargs={'return_layer_dict': RETURN_LAYERS, 'in_channels_list': [256, 512, 1024, 2048], 'out_channels': 256,
                                         'analysis_config': {'analyzes_after_compress': True,
                                                             'analyzer_configs': [{'key': 'FileSizeAnalyzer', 'kwargs': {'unit': 'KB'}}]},
                                         'analyzable_layer_key': 'bottleneck_layer'},
                    start_ckpt_file_path=None)


@pytest.fixture(scope='module')
def config_model(S):
    from sc2bench_amd import dense
    return dense.faster_rcnn_model(BACKBONE_CONFIG, **MODEL_KWARGS)


def _small_model(S, **kwargs):
    """a Faster R-CNN the CPU can run: a stand-in body (four strided convs) under the real FPN, RPN and RoI heads"""
    from sc2bench_amd import dense, detection

    class Codec(S.CompressionModel):
        def __init__(self):
            super().__init__()
            self.conv = nn.Conv2d(3, 8, 3, stride=4, padding=1)

        def forward(self, x):
            return self.conv(x)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.bottleneck_layer = Codec()
            self.layer2 = nn.Conv2d(8, 16, 3, stride=2, padding=1)
            self.layer3 = nn.Conv2d(16, 32, 3, stride=2, padding=1)
            self.layer4 = nn.Conv2d(32, 64, 3, stride=2, padding=1)
            self.inplanes = 64
    torch.manual_seed(3)
    bf = dense.backbone_with_fpn(Net(), return_layer_dict=RETURN_LAYERS, in_channels_list=[8, 16, 32, 64], out_channels=16,
                                 analyzable_layer_key='bottleneck_layer')
    return dense.BaseRCNN(detection.FasterRCNN(bf, 91, **kwargs))


def test_faster_rcnn_model_builds_without_torchvision(S, config_model):
    """fails on the parent commit: `faster_rcnn_model` raised ImportError there"""
    from sc2bench_amd import dense, detection
    with pytest.raises(ImportError):
        import torchvision.models.detection  # noqa: F401
    m = config_model
    assert isinstance(m, dense.BaseRCNN) and isinstance(m.rpn, detection.RegionProposalNetwork)
    assert isinstance(m.roi_heads, detection.RoIHeads) and isinstance(m.transform, detection.GeneralizedRCNNTransform)
    assert m.transform.min_size == (800,) and m.transform.max_size == 1333
    assert m.rpn.nms_thresh == 0.7 and m.rpn._pre_nms_top_n['testing'] == 1000 and m.rpn._post_nms_top_n['testing'] == 1000
    assert m.roi_heads.score_thresh == 0.05 and m.roi_heads.nms_thresh == 0.5 and m.roi_heads.detections_per_img == 100
    assert m.roi_heads.box_coder.weights == (10.0, 10.0, 5.0, 5.0) and m.rpn.box_coder.weights == (1.0, 1.0, 1.0, 1.0)
    assert S.FasterRCNN is detection.FasterRCNN and S.batched_nms is detection.batched_nms
    sd = m.state_dict()
    assert sd['rpn.head.cls_logits.weight'].shape == (3, 256, 1, 1) and sd['rpn.head.bbox_pred.weight'].shape == (12, 256, 1, 1)
    assert sd['roi_heads.box_head.fc6.weight'].shape == (1024, 256 * 49) and sd['roi_heads.box_head.fc7.weight'].shape == (1024, 1024)
    assert sd['roi_heads.box_predictor.cls_score.weight'].shape == (91, 1024)
    assert sd['roi_heads.box_predictor.bbox_pred.weight'].shape == (364, 1024)


def test_state_dict_names_are_torchvisions(config_model):
    with open(os.path.join(HERE, 'golden', 'faster_rcnn_keys.txt')) as f:
        want = [ln.strip() for ln in f if ln.strip() and not ln.startswith('#')]
    got = [k for k in config_model.state_dict().keys() if not k.startswith('backbone.body.')]
    assert sorted(got) == sorted(want)


def test_old_rpn_head_keys_load(S):
    from sc2bench_amd import detection
    torch.manual_seed(0)
    head = detection.RPNHead(16, 3)
    sd = {k: torch.randn_like(v) for k, v in head.state_dict().items()}
    old = OrderedDict((k.replace('conv.0.0.', 'conv.'), v) for k, v in sd.items())
    assert 'conv.weight' in old and 'conv.0.0.weight' not in old
    head.load_state_dict(old)
    assert all(torch.equal(head.state_dict()[k], v) for k, v in sd.items())
    rpn = detection.RegionProposalNetwork(detection.AnchorGenerator(((32,),), ((0.5, 1.0, 2.0),)), detection.RPNHead(16, 3))
    rpn.load_state_dict(OrderedDict(('head.' + k, v) for k, v in old.items()))        # through a parent's prefix
    assert torch.equal(rpn.head.conv[0][0].weight, sd['conv.0.0.weight'])


def test_anchor_known_answers(S):
    from sc2bench_amd import detection
    ag = detection.AnchorGenerator(((32,), (64,), (128,), (256,), (512,)), ((0.5, 1.0, 2.0),) * 5)
    assert ag.num_anchors_per_location() == [3] * 5
    assert ag.cell_anchors[0].tolist() == [[-23, -11, 23, 11], [-16, -16, 16, 16], [-11, -23, 11, 23]]
    assert ag.cell_anchors[4].tolist() == [[-362, -181, 362, 181], [-256, -256, 256, 256], [-181, -362, 181, 362]]
    images = detection.ImageList(torch.zeros(2, 3, 64, 96), [(60, 90), (64, 96)])
    feats = [torch.zeros(2, 4, 16, 24), torch.zeros(2, 4, 8, 12)]
    ag2 = detection.AnchorGenerator(((32,), (64,)), ((0.5, 1.0, 2.0),) * 2)
    per_image = ag2(images, feats)
    assert len(per_image) == 2 and per_image[0].shape == (16 * 24 * 3 + 8 * 12 * 3, 4)
    a = per_image[0]
    assert a[:3].tolist() == ag2.cell_anchors[0].tolist()                             # (y, x, anchor): anchors fastest,
    assert a[3:6].tolist() == (ag2.cell_anchors[0] + torch.tensor([4.0, 0, 4, 0])).tolist()      # then x (stride 64 // 16 = 4),
    assert a[24 * 3:24 * 3 + 3].tolist() == (ag2.cell_anchors[0] + torch.tensor([0.0, 4, 0, 4])).tolist()      # then y
    assert a[16 * 24 * 3 + 3:16 * 24 * 3 + 6].tolist() == (ag2.cell_anchors[1] + torch.tensor([8.0, 0, 8, 0])).tolist()


def test_transform_sizes_and_postprocess(S):
    """Size arithmetic by the stated rule: scale = min(min_size / min(h, w), max_size / max(h, w)) and F.interpolate's own
    floor(side * scale) under recompute_scale_factor=True.  For 480 x 640 that is 800 x 1066 (640 * 800 / 480 = 1066.67 -> floor),
    padded to 800 x 1088; a rounding rule would give 1067, the floor the interpolation applies gives 1066."""
    from sc2bench_amd import detection
    t = detection.GeneralizedRCNNTransform(800, 1333, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]).eval()
    assert t.resized_size(480, 640) == (800, 1066)
    assert t.resized_size(640, 480) == (1066, 800)
    assert t.resized_size(800, 1216) == (800, 1216)
    assert t.resized_size(400, 1000) == (533, 1333)                     # the longer side limits: scale 1.333
    torch.manual_seed(0)
    imgs = [torch.rand(3, 48, 64), torch.rand(3, 60, 40)]
    t2 = detection.GeneralizedRCNNTransform(80, 133, [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]).eval()
    il, _ = t2(imgs)
    assert il.image_sizes == [t2.resized_size(48, 64), t2.resized_size(60, 40)] == [(80, 106), (120, 80)]
    assert tuple(il.tensors.shape) == (2, 3, 128, 128)                   # padded to multiples of 32
    assert torch.all(il.tensors[0, :, 80:, :] == 0) and torch.all(il.tensors[0, :, :, 106:] == 0)
    mean, std = torch.tensor(t2.image_mean)[:, None, None], torch.tensor(t2.image_std)[:, None, None]
    want = torch.nn.functional.interpolate(((imgs[0] - mean) / std)[None], size=(80, 106), mode='bilinear', align_corners=False)[0]
    assert torch.allclose(il.tensors[0, :, :80, :106], want, atol=1e-6)
    big = detection.GeneralizedRCNNTransform(800, 1333, t.image_mean, t.image_std).eval()
    il, _ = big([torch.rand(3, 480, 640)])
    assert il.image_sizes == [(800, 1066)] and tuple(il.tensors.shape) == (1, 3, 800, 1088)
    # postprocess: boxes in the resized image's pixels back to the original's, per axis
    res = [{'boxes': torch.tensor([[0.0, 0.0, 106.0, 80.0], [53.0, 20.0, 79.5, 60.0]])}]
    out = t2.postprocess(res, [(80, 106)], [(48, 64)])
    assert torch.allclose(out[0]['boxes'], torch.tensor([[0.0, 0.0, 64.0, 48.0], [32.0, 12.0, 48.0, 36.0]]), atol=1e-5)


_NMS_CASES = RD.nms_cases()


@pytest.mark.parametrize('case', _NMS_CASES, ids=[c[0] for c in _NMS_CASES])
def test_torch_op_nms_equals_reference(S, case):
    """the package's torch-op batched NMS (the CPU path, and the A/B path on the device) on the GPU tests' inputs: the same kept
    indices in the same order as the sequential float32 reference"""
    from sc2bench_amd import detection
    _, boxes, scores, groups, thr = case
    got = detection.batched_nms(torch.from_numpy(boxes), torch.from_numpy(scores), torch.from_numpy(groups), thr)
    assert got.dtype == torch.int64 and got.tolist() == RD.batched_nms_ref(boxes, scores, groups, thr).tolist()
    if groups.max() == 0:
        assert detection.nms(torch.from_numpy(boxes), torch.from_numpy(scores), thr).tolist() == got.tolist()


@pytest.mark.parametrize('bf16', [False, True], ids=['f32', 'bf16'])
@pytest.mark.parametrize('K,seed', [(1, 11), (37, 12), (300, 13)])
@pytest.mark.parametrize('P', [7, 2])
def test_torch_op_roi_align_equals_reference(S, P, K, seed, bf16):
    """the torch-op RoIAlign (f32 arithmetic) against the float64 reference on the same rounded inputs, within the GPU test's
    bound 2^-12 * max|x|"""
    from sc2bench_amd import detection
    C = 8
    feats = RD.roi_features(C, seed=C)
    tf = [torch.from_numpy(f) for f in feats]
    if bf16:
        tf = [f.to(torch.bfloat16) for f in tf]
        feats = [f.float().numpy() for f in tf]
    for mode in ('mixed', 'one', 'skip'):
        rois, levels, dropped = RD.roi_cases(K, seed, P, 2, mode)
        assert dropped <= 0.05 * K
        want = RD.roi_align_ref(feats, RD.SCALES, rois, levels, P, 2)
        got = detection.multiscale_roi_align(tf, RD.SCALES, torch.from_numpy(rois), torch.from_numpy(levels), P, 2)
        assert got.dtype == torch.float32 and tuple(got.shape) == (K, C, P, P)
        bound = 2.0 ** -12 * max(np.abs(f).max() for f in feats)
        assert np.abs(got.numpy().astype(np.float64) - want).max() <= bound
    single = detection.roi_align(tf[0], torch.from_numpy(rois[levels == 0]), P, RD.SCALES[0], 2)
    assert torch.equal(single.float(), got[torch.from_numpy(levels == 0)].to(single.dtype).float())


def test_cpu_forward_returns_well_formed_detections(S):
    model = _small_model(S, min_size=64, max_size=96, box_score_thresh=0.0).eval()
    torch.manual_seed(1)
    with torch.no_grad():
        out = model([torch.rand(3, 64, 96)])
    assert len(out) == 1 and sorted(out[0].keys()) == ['boxes', 'labels', 'scores']
    boxes, labels, scores = out[0]['boxes'], out[0]['labels'], out[0]['scores']
    d = boxes.shape[0]
    assert 0 < d <= 100 and boxes.shape == (d, 4) and labels.shape == (d,) and scores.shape == (d,)
    assert labels.dtype == torch.int64 and labels.min() >= 1 and labels.max() <= 90
    assert torch.all(scores[:-1] >= scores[1:]) and torch.all(scores > 0)
    assert boxes[:, 0::2].min() >= 0 and boxes[:, 0::2].max() <= 96 and boxes[:, 1::2].min() >= 0 and boxes[:, 1::2].max() <= 64
    assert torch.all(boxes[:, 2] > boxes[:, 0]) and torch.all(boxes[:, 3] > boxes[:, 1])
    with torch.no_grad():       # a second image of another size in the batch: per-image results, rescaled per image
        out2 = model([torch.rand(3, 64, 96), torch.rand(3, 50, 70)])
    assert len(out2) == 2 and out2[1]['boxes'][:, 0::2].max() <= 70 and out2[1]['boxes'][:, 1::2].max() <= 50


def test_pooler_takes_three_maps_under_the_configs_names(S, config_model):
    """The reference's configs name the pyramid '1', '2', '3', '4', 'pool'; FasterRCNN's default pooler asks for '0'..'3': maps
    '1', '2', '3' (strides 4, 8, 16) reach it and large RoIs clamp to stride 16.  Kept as the reference behaves."""
    pool = config_model.roi_heads.box_roi_pool
    assert pool.featmap_names == ['0', '1', '2', '3'] and pool.output_size == (7, 7) and pool.sampling_ratio == 2
    feats = OrderedDict((name, torch.zeros(1, 8, 256 // s, 320 // s)) for name, s in zip(['1', '2', '3', '4', 'pool'], [4, 8, 16, 32, 64]))
    used = pool.filtered(feats)
    assert [tuple(f.shape[-2:]) for f in used] == [(64, 80), (32, 40), (16, 20)]
    pool.setup_scales(used, [(256, 320)])
    assert pool.scales == [0.25, 0.125, 0.0625] and (pool.map_levels.k_min, pool.map_levels.k_max) == (2, 4)
    boxes = torch.tensor([[0.0, 0, 20, 20], [0, 0, 111, 111], [0, 0, 113, 113], [0, 0, 224, 224], [0, 0, 300, 250], [0, 0, 448, 448]])
    # level = floor(4 + log2(sqrt(area) / 224) + 1e-6) clamped to [2, 4], minus 2: 112 is the 3 -> 2 ... boundary of level 3
    assert pool.map_levels([boxes]).tolist() == [0, 0, 1, 2, 2, 2]
    out = pool(feats, [boxes], [(256, 320)])
    assert tuple(out.shape) == (6, 8, 7, 7)


def test_training_mode_is_not_built(S):
    from sc2bench_amd import detection
    model = _small_model(S, min_size=64, max_size=96).train()
    images = detection.ImageList(torch.rand(1, 3, 64, 96), [(64, 96)])
    feats = model.backbone(images.tensors)
    targets = [{'boxes': torch.tensor([[4.0, 4.0, 40.0, 40.0]]), 'labels': torch.tensor([3])}]
    with pytest.raises(NotImplementedError, match='matcher.*samplers.*losses'):
        model.rpn(images, feats, targets)
    with pytest.raises(NotImplementedError, match='matcher.*samplers.*losses'):
        model.roi_heads(feats, [targets[0]['boxes']], images.image_sizes, targets)
    with pytest.raises(ValueError, match='targets should not be None'):
        model.rpn(images, feats)
    with pytest.raises(NotImplementedError):
        model([torch.rand(3, 64, 96)], targets)
