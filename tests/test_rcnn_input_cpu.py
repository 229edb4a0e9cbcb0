"""CPU: the host side of the input-compression baselines for detection and segmentation -- the two C-ABI symbols of
csrc/rcnn_input.hip and their switch, `RCNNTransformWithCompression`'s host path against a step-by-step restatement from Pillow calls,
which lists may reach the kernels at all, the two wrappers, the builders, `config.build_model` and `evaluation.test_only`."""
import io
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import coco_cases as CC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
ACC = [{'key': 'FileSizeAccumulator', 'kwargs': {'unit': 'KB'}}]


def _codec(S, **kw):
    kw = dict(dict(format='JPEG', quality=90), **kw)
    return S.transforms.Compose([S.PILImageModule(returns_file_size=True, **kw)])


def _transform(S, codec=None, device='cpu', **kw):
    base = S.GeneralizedRCNNTransform(80, 133, MEAN, STD)
    t = S.RCNNTransformWithCompression(base, device, _codec(S) if codec is None else codec, ACC, **kw)
    t.eval()
    t.activate_analysis()
    return t


def _images(sizes=((37, 53), (60, 40), (100, 120)), seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(3, h, w, generator=g) for h, w in sizes]


def test_symbols_switch_and_cpu_refusal(S):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sc2_bottleneck.h')).read(), flags=re.S)
    for name in ('sc2_rcnn_resize_u8', 'sc2_rcnn_normalize_pad'):
        assert re.search(r'\b' + name + r'\s*\(', text), name + ' is not declared'
        assert name in S.hip.ABI_SYMBOLS
        assert hasattr(S.hip.lib(), name)
    assert "'rcnn_input.hip'" in open(os.path.join(ROOT, 'sc2-benchmark_amd', 'build.py')).read()
    assert S.hip.lib().sc2_abi_version() == 51
    assert isinstance(S.hip.HostPolicy.rcnn_input_hip, bool)
    before = S.hip.host_policy.rcnn_input_hip
    try:
        S.hip.configure(rcnn_input_hip=not before)
        assert S.hip.host_policy.rcnn_input_hip is (not before)
    finally:
        S.hip.configure(rcnn_input_hip=before)
    with pytest.raises(S.hip.Sc2Error, match='no CPU fallback'):
        S.hip.rcnn_resize_u8(torch.zeros(3, 8, 8), 16, 16)
    with pytest.raises(S.hip.Sc2Error, match='no CPU fallback'):
        S.hip.rcnn_normalize_pad(torch.zeros(3, 8, 8, dtype=torch.uint8), MEAN, STD, torch.zeros(3, 32, 32))


def _restated(images, quality=90, min_size=80, max_size=133, divisible=32):
    """The transform step by step from torch's interpolate and Pillow calls: -> (batch, image sizes, file sizes in bytes)"""
    from PIL import Image
    outs, sizes, file_sizes = [], [], []
    for x in images:
        h, w = x.shape[-2:]
        scale = min(float(min_size) / min(h, w), float(max_size) / max(h, w))
        y = F.interpolate(x[None], scale_factor=scale, mode='bilinear', recompute_scale_factor=True, align_corners=False)[0]
        arr = y.mul(255).byte().permute(1, 2, 0).contiguous().numpy()
        buf = io.BytesIO()
        Image.fromarray(arr, mode='RGB').save(buf, format='JPEG', quality=quality)
        file_sizes.append(len(buf.getvalue()))
        dec = np.asarray(Image.open(io.BytesIO(buf.getvalue())))
        z = torch.from_numpy(dec.copy()).permute(2, 0, 1).to(torch.float32).div(255)
        outs.append((z - torch.tensor(MEAN)[:, None, None]) / torch.tensor(STD)[:, None, None])
        sizes.append((int(y.shape[-2]), int(y.shape[-1])))
    Hp = int(math.ceil(max(s[0] for s in sizes) / divisible) * divisible)
    Wp = int(math.ceil(max(s[1] for s in sizes) / divisible) * divisible)
    batch = torch.zeros(len(images), 3, Hp, Wp)
    for i, o in enumerate(outs):
        batch[i, :, :o.shape[1], :o.shape[2]] = o
    return batch, sizes, file_sizes


def test_host_path_equals_the_restatement(S):
    pytest.importorskip('PIL')
    images = _images()
    t = _transform(S)
    out, targets = t(images)
    batch, sizes, file_sizes = _restated(images)
    assert targets is None
    assert out.image_sizes == sizes == [(80, 114), (120, 80), (80, 96)]
    assert tuple(out.tensors.shape) == (3, 3, 128, 128)
    assert torch.equal(out.tensors, batch)
    assert t.analyzers[0].file_size_list == [n / 1024 for n in file_sizes]
    # training mode: the same pixels, nothing analysed
    t.clear_analysis()
    t.train()
    assert torch.equal(t(images)[0].tensors, batch) and t.analyzers[0].file_size_list == []
    with pytest.raises(ValueError, match='3d tensors'):
        t([torch.rand(1, 3, 8, 8)])


def test_targets_boxes_are_resized(S):
    pytest.importorskip('PIL')
    images = _images(((40, 60),))
    boxes = torch.tensor([[10.0, 4.0, 30.0, 20.0]])
    target = {'boxes': boxes, 'labels': torch.tensor([1])}
    out, targets = _transform(S)(images, [target])
    assert out.image_sizes == [(80, 120)]
    assert torch.equal(targets[0]['boxes'], boxes * 2.0) and torch.equal(targets[0]['labels'], target['labels'])
    assert torch.equal(target['boxes'], boxes)       # the caller's dictionary is not modified


def test_shape_changing_post_transform_is_refused(S):
    pytest.importorskip('PIL')
    t = _transform(S, post_transform=lambda x: x[:, :-1])
    with pytest.raises(AssertionError, match='should not change tensor shape'):
        t(_images(((40, 60),)))


class StubCompressionModel(torch.nn.Module):
    """compress: the padded image itself as the `strings`; decompress: plus 0.25"""

    def __init__(self):
        super().__init__()
        self.seen = []

    def compress(self, x):
        self.seen.append(tuple(x.shape))
        return {'strings': [x.clone()], 'shape': tuple(x.shape[-2:])}

    def decompress(self, strings, shape):
        assert tuple(strings[0].shape[-2:]) == tuple(shape)
        return {'x_hat': strings[0] + 0.25}


class Recorder(object):
    def __init__(self):
        self.objs = []

    def analyze(self, obj):
        self.objs.append(obj)


def test_compress_by_model_pads_analyses_and_crops(S):
    model = StubCompressionModel()
    base = S.GeneralizedRCNNTransform(80, 133, MEAN, STD)
    t = S.RCNNTransformWithCompression(base, 'cpu', None, [], analyzes_after_compress=True, compression_model=model,
                                       adaptive_pad_kwargs={'factor': 64})
    t.eval()
    t.activate_analysis()
    rec = Recorder()
    t.analyzers = [rec]
    images = _images(((40, 60),))
    out, _ = t(images)
    assert model.seen == [(1, 3, 128, 128)] and out.image_sizes == [(80, 120)]       # 80 x 120 padded to multiples of 64
    obj, h, w = rec.objs[0]
    assert (h, w) == (80, 120) and obj['shape'] == (128, 128)
    resized = F.interpolate(images[0][None], scale_factor=2.0, mode='bilinear', recompute_scale_factor=True, align_corners=False)[0]
    assert torch.equal(out.tensors[0, :, :80, :120], t.normalize(resized + 0.25))
    # without the pad the object is analysed alone; with analysis after compression off, nothing is
    t2 = S.RCNNTransformWithCompression(base, 'cpu', None, [], analyzes_after_compress=True, compression_model=StubCompressionModel())
    t2.eval()
    t2.activate_analysis()
    t2.analyzers = [Recorder()]
    t2(images)
    assert isinstance(t2.analyzers[0].objs[0], dict)
    t3 = S.RCNNTransformWithCompression(base, 'cpu', None, [], compression_model=StubCompressionModel(), uses_cpu4compression_model=True)
    t3.eval()
    t3.activate_analysis()
    t3.analyzers = [Recorder()]
    assert t3(images)[0].image_sizes == [(80, 120)] and t3.analyzers[0].objs == []


class OnDevice(torch.Tensor):
    """A host tensor that says it is on a HIP device: the gate's decision can be tested where no device exists."""
    is_cuda = property(lambda self: True)


def _on_device(images):
    return [img.as_subclass(OnDevice) for img in images]


def test_only_eligible_lists_reach_the_kernels(S, monkeypatch):
    pytest.importorskip('PIL')

    def refuse(*a, **k):
        raise AssertionError('hip was reached')
    monkeypatch.setattr(S.hip, 'rcnn_resize_u8', refuse)
    monkeypatch.setattr(S.hip.host_policy, 'rcnn_input_hip', True)
    monkeypatch.setattr(S.hip.host_policy, 'jpeg_image_hip', True)
    images = _images(((37, 53), (60, 40)))
    fake = _on_device(images)
    # the eligible list: the plan is made, and `forward` goes to the kernel (here: to the stub that refuses)
    t = _transform(S)
    assert t._kernel_plan(fake) == (90, [(80, 114), (120, 80)])
    assert _transform(S, codec=S.PILImageModule(returns_file_size=True, format='JPEG', quality=75))._kernel_plan(fake)[0] == 75
    with pytest.raises(AssertionError, match='hip was reached'):
        t(fake)
    expected = _restated(images)[0]

    def host(transform, imgs):
        assert transform._kernel_plan(imgs) is None
        return transform(imgs)[0].tensors
    # one condition at a time
    tr = _transform(S)
    tr.train()
    assert torch.equal(host(tr, fake), expected)                                                     # training mode
    assert torch.equal(host(_transform(S, post_transform=lambda x: x), fake), expected)              # a post_transform
    assert torch.equal(host(_transform(S, pre_transform=lambda x: x), fake), expected)               # a pre_transform
    tm = _transform(S, compression_model=StubCompressionModel())
    assert tm._kernel_plan(fake) is None and tm(fake)[0].image_sizes == [(80, 114), (120, 80)]       # a compression model
    assert host(_transform(S, codec=_codec(S, optimize=True)), fake).shape == expected.shape         # optimize=True
    try:
        webp = host(_transform(S, codec=_codec(S, format='WEBP')), fake)                             # WebP
        assert webp.shape == expected.shape
    except (KeyError, OSError):       # a Pillow without the WebP codec: the decision alone
        assert _transform(S, codec=_codec(S, format='WEBP'))._kernel_plan(fake) is None
    assert _transform(S, codec=S.PILImageModule(format='JPEG', quality=90))._kernel_plan(fake) is None   # no file size reported
    assert torch.equal(host(_transform(S), images), expected)                                        # CPU images
    assert torch.equal(host(_transform(S), [fake[0], images[1]]), expected)                          # one CPU image among them
    assert _transform(S)._kernel_plan(_on_device([torch.rand(1, 37, 53)])) is None                   # one channel
    assert _transform(S)._kernel_plan(_on_device([torch.rand(3, 37, 53).double()])) is None          # not float32
    wide = _on_device([torch.rand(3, 8, S.hip.JPEG_IMAGE_MAX_SIDE + 1)])
    assert _transform(S)._kernel_plan(wide) is None                                                  # an input side > 2048
    big = S.RCNNTransformWithCompression(S.GeneralizedRCNNTransform(2100, 4000, MEAN, STD), 'cpu', _codec(S), ACC).eval()
    assert big.resized_size(37, 53)[0] > S.hip.JPEG_IMAGE_MAX_SIDE and big._kernel_plan(fake) is None    # a resized side > 2048
    fixed = _transform(S)
    fixed.fixed_size = (96, 64)
    assert fixed._kernel_plan(fake) is None                                                          # fixed_size
    monkeypatch.setattr(S.hip.host_policy, 'rcnn_input_hip', False)
    assert torch.equal(host(_transform(S), fake), expected)                                          # switch off
    monkeypatch.setattr(S.hip.host_policy, 'rcnn_input_hip', True)
    monkeypatch.setattr(S.hip.host_policy, 'jpeg_image_hip', False)
    assert torch.equal(host(_transform(S), fake), expected)                                          # the codec's switch off


class TinyDetector(torch.nn.Module):
    def __init__(self, S):
        super().__init__()
        self.transform = S.GeneralizedRCNNTransform(80, 133, MEAN, STD)

    def forward(self, images):
        return self.transform(images)[0]


def test_detection_wrapper_replaces_the_transform_and_delegates(S):
    pytest.importorskip('PIL')
    assert S.WRAPPER_CLASS_DICT['InputCompressionDetectionModel'] is S.InputCompressionDetectionModel
    inner = TinyDetector(S)
    w = S.InputCompressionDetectionModel(inner, 'cpu', codec_encoder_decoder=_codec(S), adaptive_pad_config=None,
                                         analysis_config={'analyzer_configs': ACC, 'analyzes_after_compress': True})
    t = inner.transform
    assert isinstance(t, S.RCNNTransformWithCompression) and w.detection_model is inner and w.analyzers == []
    assert t.min_size == (80,) and t.max_size == 133 and t.analyzes_after_compress is True and len(t.analyzers) == 1
    w.eval()
    images = _images(((37, 53),))
    w(images)
    assert t.analyzers[0].file_size_list == []             # analysis is off until it is activated
    w.activate_analysis()
    assert w.activated_analysis and t.activated_analysis
    out = w(images)
    assert torch.equal(out.tensors, _restated(images)[0]) and len(t.analyzers[0].file_size_list) == 1
    w.analyze(2048)
    assert t.analyzers[0].file_size_list[-1] == 2.0
    w.summarize()
    w.clear_analysis()
    assert t.analyzers[0].file_size_list == []
    w.deactivate_analysis()
    assert not w.activated_analysis and not t.activated_analysis
    w.use_cpu4compression()       # no compression model: nothing to move
    model = StubCompressionModel()
    w2 = S.InputCompressionDetectionModel(TinyDetector(S), 'cpu', compression_model=model, uses_cpu4compression_model=True)
    w2.use_cpu4compression()
    assert w2.detection_model.transform.compression_model is model and w2.detection_model.transform.uses_cpu4compression_model


def _detection_config(S):
    """configs/coco2017/input_compression/jpeg-faster_rcnn_resnet50_fpn.yaml as the loader hands it on (tags evaluated), at a small size"""
    return {'key': 'InputCompressionDetectionModel',
            'kwargs': {'codec_encoder_decoder': _codec(S), 'analysis_config': {'analyzer_configs': ACC, 'analyzes_after_compress': True},
                       'adaptive_pad_config': None, 'pre_transform': None, 'post_transform': None},
            'detection_model': {'key': 'fasterrcnn_resnet50_fpn',
                                'kwargs': {'pretrained': True, 'progress': True, 'min_size': 80, 'max_size': 133}}}


def _segmentation_config(S):
    """configs/pascal_voc2012/input_compression/jpeg-deeplabv3_resnet50.yaml likewise (no checkpoint address)"""
    T = S.transforms
    return {'key': 'CodecInputCompressionSegmentationModel',
            'kwargs': {'codec_encoder_decoder': _codec(S), 'analysis_config': {'analyzer_configs': ACC},
                       'post_transform': T.Compose([T.ToTensor(), T.Normalize(mean=MEAN, std=STD)])},
            'segmentation_model': {'key': 'deeplabv3_resnet50', 'kwargs': {'pretrained': True, 'num_classes': 21, 'aux_loss': True}}}


@pytest.fixture(scope='module')
def built(S):
    from sc2bench_amd import config as C
    torch.manual_seed(0)
    return C.build_model(_detection_config(S), torch.device('cpu')), C.build_model(_segmentation_config(S), torch.device('cpu'))


def test_build_model_builds_both_wrappers(S, built):
    det, seg = built
    assert isinstance(det, S.InputCompressionDetectionModel) and isinstance(det.detection_model, S.FasterRCNN)
    assert isinstance(det.detection_model.transform, S.RCNNTransformWithCompression)
    assert det.detection_model.transform.min_size == (80,) and det.detection_model.roi_heads.box_predictor.cls_score.out_features == 91
    keys = set(det.detection_model.state_dict())
    listed = [l.strip() for l in open(os.path.join(ROOT, 'tests', 'golden', 'faster_rcnn_keys.txt')) if l.strip() and not l.startswith('#')]
    assert set(listed) <= keys and 'backbone.body.layer4.2.bn3.running_var' in keys
    assert isinstance(seg, S.CodecInputCompressionSegmentationModel) and isinstance(seg.segmentation_model, S.BaseSegmentationModel)
    assert seg.segmentation_model.aux_classifier is not None and len(seg.analyzers) == 1
    skeys = set(seg.segmentation_model.state_dict())
    assert {'backbone.layer4.2.conv3.weight', 'classifier.4.weight', 'aux_classifier.4.bias'} <= skeys
    assert seg.segmentation_model.backbone.layer4[1].conv2.dilation == (4, 4)
    for name in ('fasterrcnn_resnet50_fpn',):
        assert name in S.DETECTION_MODEL_FUNC_DICT
    assert 'deeplabv3_resnet50' in S.SEGMENTATION_MODEL_FUNC_DICT
    for name in ('get_wrapped_detection_model', 'get_wrapped_segmentation_model', 'RCNNTransformWithCompression'):
        assert hasattr(S, name)


def test_pretrained_without_a_checkpoint_warns(S, caplog):
    import logging
    with caplog.at_level(logging.WARNING):
        S.fasterrcnn_resnet50_fpn(pretrained=True, num_classes=3)
    assert 'start_ckpt_file_path' in caplog.text


class EchoSegmenter(torch.nn.Module):
    def forward(self, x):
        return {'out': x}


def test_segmentation_wrapper_equals_the_reference_loop(S):
    pytest.importorskip('PIL')
    from PIL import Image
    assert S.WRAPPER_CLASS_DICT['CodecInputCompressionSegmentationModel'] is S.CodecInputCompressionSegmentationModel
    seg = S.CodecInputCompressionSegmentationModel(EchoSegmenter(), 'cpu', **_segmentation_config(S)['kwargs'])
    seg.eval()
    seg.activate_analysis()
    rng = np.random.RandomState(0)
    images = [Image.fromarray(rng.randint(0, 256, size=(33, 47, 3), dtype=np.uint8)) for _ in range(2)]
    got = seg(images)['out']
    tmp, sizes = [], []
    for img in images:        # the reference's loop
        dec, n = seg.codec_encoder_decoder(img)
        sizes.append(n / 1024)
        tmp.append(seg.post_transform(dec).unsqueeze(0))
    assert torch.equal(got, torch.hstack(tmp)) and tuple(got.shape) == (1, 6, 33, 47)
    assert seg.analyzers[0].file_size_list == sizes


def test_test_only_routes_both_wrappers(S):
    pytest.importorskip('PIL')
    from PIL import Image
    from sc2bench_amd import evaluation as E
    gt, _ = CC.random_case(21, images=2, empty=0.0)
    config = {'models': {'model': _detection_config(S)}, 'datasets': {'coco2017/val': {'coco_gt': gt}},
              'test': {'test_data_loader': {'dataset_id': 'coco2017/val', 'collate_fn': 'coco_collate_fn', 'kwargs': {'batch_size': 1}}}}
    res = E.test_only(config, torch.device('cpu'), max_samples=2)
    assert res['samples'] == 2 and len(res['stats']) == 12 and 'Average Precision' in res['summary']
    assert len(res['analysis']) == 1 and res['analysis'][0]['count'] == 2 and res['analysis'][0]['unit'] == 'KB' and res['analysis'][0]['mean'] > 0

    class Toy(torch.utils.data.Dataset):
        def __len__(self):
            return 2

        def __getitem__(self, i):
            rng = np.random.RandomState(i)
            return Image.fromarray(rng.randint(0, 256, size=(33, 33, 3), dtype=np.uint8)), torch.from_numpy(rng.randint(0, 21, size=(33, 33)))
    config = {'models': {'model': _segmentation_config(S)}, 'datasets': {'pascal_voc2012/val': Toy()},
              'test': {'test_data_loader': {'dataset_id': 'pascal_voc2012/val', 'collate_fn': 'pascal_seg_eval_collate_fn', 'kwargs': {'batch_size': 1}}}}
    res = E.test_only(config, torch.device('cpu'))
    assert res['samples'] == 2 and len(res['iou']) == 21 and res['evaluator'].mat.sum().item() == 2 * 33 * 33
    assert len(res['analysis']) == 1 and res['analysis'][0]['count'] == 2
