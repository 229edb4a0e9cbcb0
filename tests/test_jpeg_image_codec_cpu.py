"""CPU: the host side of the JPEG input-compression kernel path -- the three C-ABI symbols and the sizing helpers, the policy switch,
`PILImageModule.forward_batch` against the per-image loop, which modules and devices may reach the kernel at all, the wrapper's
list-of-images form against its loop form, and `to_tensor` of decoded uint8 pixels."""
import os
import re

import numpy as np
import pytest
import torch

import jpeg_image_cases as IC
import ref_jpeg as RJ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_and_listed(S):
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sc2_bottleneck.h')).read(), flags=re.S)
    for name in ('sc2_jpeg_image_max_bytes', 'sc2_jpeg_image_workspace_bytes', 'sc2_jpeg_image_codec'):
        assert re.search(r'\b' + name + r'\s*\(', text), name + ' is not declared'
        assert name in S.hip.ABI_SYMBOLS
        assert hasattr(S.hip.lib(), name)
    assert "'jpeg_image.hip'" in open(os.path.join(ROOT, 'sc2-benchmark_amd', 'build.py')).read()
    for name, value in (('SC2_JPEG_IMAGE_MAX_SIDE', S.hip.JPEG_IMAGE_MAX_SIDE), ('SC2_JPEG_IMAGE_CHUNK_BLOCKS', S.hip.JPEG_IMAGE_CHUNK_BLOCKS)):
        assert int(re.search(r'#define\s+' + name + r'\s+(\d+)', text).group(1)) == value
    assert S.hip.JPEG_IMAGE_MAX_SIDE >= 1344
    assert 6 * (S.hip.JPEG_IMAGE_MAX_SIDE // 16) ** 2 * RJ.MAX_BLOCK_BITS < 2 ** 31


def test_sizing_helpers(S):
    lib, top = S.hip.lib(), S.hip.JPEG_IMAGE_MAX_SIDE
    for C, mode in ((1, 'L'), (3, 'RGB')):
        for H, W in ((1, 1), (65, 64), (224, 224), (16, top)):
            assert lib.sc2_jpeg_image_max_bytes(C, H, W) == RJ.max_bytes(mode, H, W)
            assert S.hip.jpeg_image_max_bytes(C, H, W) == RJ.max_bytes(mode, H, W)
    for C, H, W in ((2, 8, 8), (3, 0, 8), (3, 8, 0), (3, top + 1, 8), (1, 8, top + 1)):
        assert lib.sc2_jpeg_image_max_bytes(C, H, W) == -1 and lib.sc2_jpeg_image_workspace_bytes(1, C, H, W) == -1
    with pytest.raises(S.hip.Sc2Error, match=str(top)):
        S.hip.jpeg_image_max_bytes(3, top + 1, 8)
    one, five = (lib.sc2_jpeg_image_workspace_bytes(B, 3, 224, 224) for B in (1, 5))
    assert one > 0 and five > one
    assert lib.sc2_jpeg_image_workspace_bytes(0, 3, 8, 8) == -1
    assert 0 < lib.sc2_jpeg_image_workspace_bytes(1, 1, 1, 1) < lib.sc2_jpeg_image_workspace_bytes(2, 1, 1, 1)


def test_policy_field_and_cpu_refusal(S):
    assert isinstance(S.hip.HostPolicy.jpeg_image_hip, bool)
    before = S.hip.host_policy.jpeg_image_hip
    try:
        S.hip.configure(jpeg_image_hip=not before)
        assert S.hip.host_policy.jpeg_image_hip is (not before)
    finally:
        S.hip.configure(jpeg_image_hip=before)
    with pytest.raises(S.hip.Sc2Error, match='no CPU fallback'):
        S.hip.jpeg_image_codec(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), 90)


def _image(C, H, W, content='gradient', seed=0):
    from PIL import Image
    arr = IC.pixels(C, H, W, content, seed)
    return Image.fromarray(arr[0] if C == 1 else np.ascontiguousarray(arr.transpose(1, 2, 0)))


def _same_images(a, b):
    return len(a) == len(b) and all(x.mode == y.mode and x.size == y.size and (np.asarray(x) == np.asarray(y)).all() for x, y in zip(a, b))


@pytest.mark.parametrize('switch', [False, True])
def test_forward_batch_equals_the_per_image_loop_on_cpu(S, monkeypatch, switch):
    """A CPU device never takes the kernel path, whatever the switch says."""
    pytest.importorskip('PIL')
    monkeypatch.setattr(S.hip.host_policy, 'jpeg_image_hip', switch)

    def refuse(*a, **k):
        raise AssertionError('hip was reached')
    monkeypatch.setattr(S.hip, 'jpeg_image_codec', refuse)
    m = S.PILImageModule(returns_file_size=True, format='JPEG', quality=90)
    commented = _image(3, 24, 40, seed=3)
    commented.info['comment'] = b'a comment the writer copies into the file'
    lists = {'equal': [_image(3, 24, 40, seed=s) for s in range(3)],
             'mixed': [_image(3, 24, 40), _image(3, 17, 33), _image(3, 24, 40, seed=2)],
             'grey': [_image(1, 30, 20, seed=s) for s in range(2)],
             'commented': [_image(3, 24, 40, seed=3), commented]}
    for name, images in lists.items():
        decoded, sizes = m.forward_batch(images, torch.device('cpu'))
        loop = [m(img) for img in images]
        assert isinstance(decoded, list) and _same_images(decoded, [d for d, _ in loop]), name
        assert sizes == [n for _, n in loop] and all(n > 0 for n in sizes), name
    # the comment is part of the file Pillow writes: the same pixels cost more bytes, which the kernel's size would not show
    sizes = m.forward_batch(lists['commented'], torch.device('cpu'))[1]
    assert sizes[1] > sizes[0]
    assert m._kernel_quality(lists['commented'], torch.device('cuda', 0)) is None


def test_only_plain_jpeg_of_one_size_is_eligible(S, monkeypatch):
    """`_jpeg_quality` is the gate `PILTensorModule` has; `_kernel_quality` adds the device, the switch and the list's conditions.
    `hip.jpeg_image_codec` is never reached for an ineligible module, list or device."""
    pytest.importorskip('PIL')
    M = S.PILImageModule
    assert M(format='JPEG', quality=90)._jpeg_quality() == 90 and M(format='jpeg')._jpeg_quality() == 75 and M(format='Jpeg', quality=1)._jpeg_quality() == 1
    refused = (dict(format='WEBP', quality=90), dict(format='PNG'), dict(format='JPEG', quality=90, optimize=True),
               dict(format='JPEG', subsampling=0), dict(format='JPEG', progressive=True), dict(format='JPEG', quality='keep'),
               dict(format='JPEG', quality=0), dict(format='JPEG', quality=101), dict(format='JPEG', quality=90.0), dict(quality=90),
               dict(format='JPEG', quality=True))
    for kwargs in refused:
        assert M(**kwargs)._jpeg_quality() is None, kwargs
        assert M(**kwargs)._jpeg_quality() == S.PILTensorModule(**kwargs)._jpeg_quality()
    assert M(open_kwargs={'formats': ['JPEG']}, format='JPEG', quality=90)._jpeg_quality() is None
    monkeypatch.setattr(S.hip.host_policy, 'jpeg_image_hip', True)

    def refuse(*a, **k):
        raise AssertionError('hip was reached')
    monkeypatch.setattr(S.hip, 'jpeg_image_codec', refuse)
    hip_dev, images = torch.device('cuda', 0), [_image(3, 16, 24, seed=s) for s in range(2)]
    assert M(format='JPEG', quality=90)._kernel_quality(images, hip_dev) == 90          # (a decision only: nothing is launched)
    assert M(format='JPEG', quality=90)._kernel_quality(images, 'cuda:0') == 90
    assert M(format='JPEG', quality=90)._kernel_quality(images, torch.device('cpu')) is None
    for kwargs in refused[:5]:
        assert M(**kwargs)._kernel_quality(images, hip_dev) is None, kwargs
    plain = M(returns_file_size=True, format='JPEG', quality=90)
    commented = _image(3, 16, 24)
    commented.info['comment'] = b'x'
    for name, ineligible in (('empty', []), ('sizes', [_image(3, 16, 24), _image(3, 24, 16)]), ('modes', [_image(3, 16, 24), _image(1, 16, 24)]),
                             ('mode', [_image(3, 16, 24).convert('CMYK')]), ('comment', [_image(3, 16, 24), commented]),
                             ('tensor', [torch.zeros(3, 16, 24, dtype=torch.uint8)])):
        assert plain._kernel_quality(ineligible, hip_dev) is None, name
    monkeypatch.setattr(S.hip.host_policy, 'jpeg_image_hip', False)
    assert plain._kernel_quality(images, hip_dev) is None
    for kwargs in (dict(format='JPEG', quality=90), dict(format='JPEG', quality=90, optimize=True), dict(format='PNG')):
        for switch in (False, True):
            monkeypatch.setattr(S.hip.host_policy, 'jpeg_image_hip', switch)
            decoded, sizes = M(returns_file_size=True, **kwargs).forward_batch(images, torch.device('cpu'))
            assert len(decoded) == 2 and all(n > 0 for n in sizes)


class _Recorder(object):
    def __init__(self):
        self.seen = []

    def analyze(self, size):
        self.seen.append(size)

    def clear(self):
        self.seen.clear()


class _Stub(torch.nn.Module):
    def forward(self, x):
        return x.float().mean(dim=(2, 3))


@pytest.mark.parametrize('composed', [False, True])
def test_through_codec_list_form_equals_the_loop_form(S, composed):
    pytest.importorskip('PIL')
    T = S.transforms
    module = S.PILImageModule(returns_file_size=True, format='JPEG', quality=90)
    codec = T.Compose([module]) if composed else module
    post = T.Compose([T.ToTensor(), T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    model = S.CodecInputCompressionClassifier(_Stub(), torch.device('cpu'), codec_encoder_decoder=codec, post_transform=post).eval()
    assert model._batch_codec() is module
    recorder = _Recorder()
    model.analyzers = [recorder]
    model.activate_analysis()
    images = [_image(3, 24, 40, seed=s) for s in range(3)]
    assert model._image_batch_codec(images) is module and model._image_batch_codec(tuple(images)) is module
    as_batch = model._through_codec(images)
    batch_sizes = list(recorder.seen)
    recorder.clear()
    # the loop form: the same wrapper around a codec that has no `forward_batch`
    loop_model = S.CodecInputCompressionClassifier(_Stub(), torch.device('cpu'), codec_encoder_decoder=lambda img: module(img), post_transform=post).eval()
    loop_model.analyzers = [recorder]
    loop_model.activate_analysis()
    assert loop_model._image_batch_codec(images) is None
    as_loop = loop_model._through_codec(images)
    assert len(batch_sizes) == 3 and batch_sizes == recorder.seen == [module(img)[1] for img in images]
    assert as_batch.shape == (1, 9, 24, 40) and torch.equal(as_batch, as_loop)
    assert torch.equal(model(images), loop_model(images))
    # what keeps the loop: a codec that reports no size, two transforms, samples that are not PIL images
    no_size = S.CodecInputCompressionClassifier(_Stub(), torch.device('cpu'), codec_encoder_decoder=S.PILImageModule(format='JPEG'), post_transform=post)
    assert no_size._image_batch_codec(images) is None
    assert S.CodecInputCompressionClassifier(_Stub(), torch.device('cpu'), codec_encoder_decoder=T.Compose([module, module]))._image_batch_codec(images) is None
    assert model._image_batch_codec(torch.zeros(2, 3, 8, 8)) is None and model._image_batch_codec([torch.zeros(3, 8, 8)]) is None
    assert model._image_batch_codec([]) is None
    model.train()
    recorder.clear()
    assert torch.equal(model._through_codec(images), as_loop)
    assert recorder.seen == []                         # no analysis in training mode, as in the loop


def test_through_codec_batches_only_a_post_transform_that_takes_pixels(S, monkeypatch):
    """The kernel path hands the wrapper a uint8 batch tensor; here `forward_batch` is replaced by one that gives the host's decoded
    pixels as such a tensor.  ToTensor (+ Normalize) runs once on that batch and is rearranged to the loop's [1, B*C, H, W].  Any
    other post_transform -- a `Resize` first, a callable of the caller's -- expects the loop's reopened PIL image: `forward_batch` is
    then not called at all.  Every expected value is the real loop form's, over PIL images."""
    pytest.importorskip('PIL')
    T = S.transforms
    module = S.PILImageModule(returns_file_size=True, format='JPEG', quality=75)
    images = [_image(3, 17, 33, seed=s) for s in range(3)]
    decoded, sizes = module.forward_batch(images, torch.device('cpu'))
    pixels = torch.from_numpy(np.stack([np.asarray(d) for d in decoded])).permute(0, 3, 1, 2).contiguous()
    calls = []
    monkeypatch.setattr(module, 'forward_batch', lambda imgs, device: calls.append(len(imgs)) or (pixels, sizes))
    normalize = T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    for post, batched in ((T.Compose([T.ToTensor(), normalize]), True), (T.Compose([T.ToTensor()]), True),
                          (T.Compose([T.ToTensor(), normalize, normalize]), False), (T.Compose([T.Resize(12), T.ToTensor(), normalize]), False),
                          (T.Compose([T.ToTensor(), T.CenterCrop(8)]), False), (T.ToTensor(), False),
                          (lambda img: T.to_tensor(img.convert('L')) * 2, False)):
        model = S.CodecInputCompressionClassifier(_Stub(), torch.device('cpu'), codec_encoder_decoder=module, post_transform=post).eval()
        loop_model = S.CodecInputCompressionClassifier(_Stub(), torch.device('cpu'), codec_encoder_decoder=lambda img: module(img),
                                                       post_transform=post).eval()
        assert model._post_transform_takes_batches() is batched and (model._image_batch_codec(images) is module) is batched
        recorder, loop_recorder = _Recorder(), _Recorder()
        for m, r in ((model, recorder), (loop_model, loop_recorder)):
            m.analyzers = [r]
            m.activate_analysis()
        del calls[:]
        got = model._through_codec(images)
        want = loop_model._through_codec(images)
        assert calls == ([3] if batched else []), post
        assert got.dtype == want.dtype and got.shape == want.shape and torch.equal(got, want), post
        assert recorder.seen == loop_recorder.seen == sizes
    # no post_transform: the decoded pixels themselves, joined as the loop joins (the loop over PIL images has no such form)
    model = S.CodecInputCompressionClassifier(_Stub(), torch.device('cpu'), codec_encoder_decoder=module, post_transform=None).eval()
    got = model._through_codec(images)
    assert got.dtype == torch.uint8 and torch.equal(got, torch.hstack([sample.unsqueeze(0) for sample in pixels]))


def test_to_tensor_of_uint8_tensors(S):
    pytest.importorskip('PIL')
    T = S.transforms
    img = _image(3, 13, 21, 'noise')
    chw = torch.from_numpy(np.asarray(img)).permute(2, 0, 1)
    assert torch.equal(T.to_tensor(chw), T.to_tensor(img)) and torch.equal(T.ToTensor()(chw.contiguous()), T.to_tensor(img))
    batch = torch.stack([chw, chw.flip(-1)])
    assert torch.equal(T.to_tensor(batch), torch.stack([T.to_tensor(chw), T.to_tensor(chw.flip(-1))]))
    grey = _image(1, 13, 21, 'noise')
    assert torch.equal(T.to_tensor(torch.from_numpy(np.asarray(grey))[None]), T.to_tensor(grey))
    every = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16)
    assert torch.equal(T.to_tensor(every), torch.arange(256, dtype=torch.float32).reshape(1, 16, 16) / 255)
    # other inputs as before: an HWC uint8 ndarray, a PIL image
    assert torch.equal(T.to_tensor(np.asarray(img)), T.to_tensor(img))
