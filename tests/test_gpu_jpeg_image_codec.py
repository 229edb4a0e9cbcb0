"""GPU: sc2_jpeg_image_codec (csrc/jpeg_image.hip) against the sequential integer restatement tests/ref_jpeg.py with NO tolerance --
the decoded pixels, the size of the file and the bytes of the entropy-coded segment --, and `PILImageModule.forward_batch` and the
input-compression wrapper that call it against the host path they replace (Pillow per image)."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_image_cases as IC

pytestmark = pytest.mark.gpu

GUARD = 256                     # sentinel bytes in front of and behind every output
SENTINEL = 0xA5


def _check(S, arr, res, quality, i=0):
    """image i of a JpegImageResult against the reference of arr [C,H,W]"""
    segment, _, decoded, size = IC.reference(arr, quality)
    header = S.hip.JPEG_HEADER_BYTES[S.hip.JPEG_RGB if arr.shape[0] == 3 else S.hip.JPEG_GREY]
    assert size == header + len(segment) + 2
    assert int(res.sizes[i]) == size, (int(res.sizes[i]), size)
    assert torch.equal(res.recon[i].cpu(), torch.from_numpy(decoded))
    if res.bytes is not None:
        assert res.bytes[i, :len(segment)].cpu().numpy().tobytes() == segment


@pytest.mark.parametrize('case', IC.CASES, ids=IC.case_id)
def test_kernel_matches_the_reference(S, dev, case):
    arr = IC.case_pixels(case)
    x = torch.from_numpy(arr[None]).to(dev)
    res = S.hip.jpeg_image_codec(x, case[4], want_bytes=True)
    assert res.recon.shape == x.shape and res.recon.dtype == torch.uint8 and res.recon.is_contiguous()
    assert res.sizes.shape == (1,) and res.sizes.dtype == torch.int32
    assert res.bytes.shape == (1, S.hip.jpeg_image_max_bytes(*case[:3])) and res.slot_bytes == res.bytes.shape[1]
    _check(S, arr, res, case[4])
    plain = S.hip.jpeg_image_codec(x, case[4])
    assert plain.bytes is None and plain.slot_bytes == 0
    _check(S, arr, plain, case[4])


@pytest.mark.parametrize('C', [3, 1])
def test_batch_of_five_different_images(S, dev, C):
    contents = ['gradient', 'noise', 'blocks', 'c137', 'gradient']
    arrs = [IC.pixels(C, 40, 56, content, seed=b) for b, content in enumerate(contents)]
    res = S.hip.jpeg_image_codec(torch.from_numpy(np.stack(arrs)).to(dev), 90, want_bytes=True)
    for b, arr in enumerate(arrs):
        _check(S, arr, res, 90, b)
    assert len(set(res.sizes.cpu().tolist())) >= 4


def test_chw_and_hwc_inputs_are_read_in_place(S, dev):
    arrs = [IC.pixels(3, 47, 49, content, seed=b) for b, content in enumerate(('gradient', 'noise'))]
    chw = torch.from_numpy(np.stack(arrs)).to(dev)
    hwc = chw.permute(0, 2, 3, 1).contiguous()
    view = hwc.permute(0, 3, 1, 2)
    assert not view.is_contiguous() and view.stride(1) == 1
    a = S.hip.jpeg_image_codec(chw, 75, want_bytes=True)
    b = S.hip.jpeg_image_codec(view, 75, want_bytes=True)
    for i, arr in enumerate(arrs):
        _check(S, arr, a, 75, i)
        _check(S, arr, b, 75, i)
    assert torch.equal(a.recon, b.recon) and torch.equal(a.sizes, b.sizes)
    # a slice: strides that are no product of the shape
    wide = torch.zeros(2, 3, 60, 70, dtype=torch.uint8, device=dev)
    wide[:, :, 5:52, 9:58] = chw
    c = S.hip.jpeg_image_codec(wide[:, :, 5:52, 9:58], 75)
    assert torch.equal(a.recon, c.recon) and torch.equal(a.sizes, c.sizes)


def _arena(n, dev):
    return torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=dev)


def _raw(S, x, quality, want_bytes, ws_fill):
    """The raw entry on outputs inside sentinel arenas and a workspace filled with `ws_fill`.  -> (recon, sizes, slots) on the host."""
    lib = S.hip.lib()
    B, C, H, W = x.shape
    dev = x.device
    recon, sizes = _arena(x.numel(), dev), _arena(4 * B, dev)
    slot = S.hip.jpeg_image_max_bytes(C, H, W)
    coded = _arena(B * slot, dev)
    ws_bytes = lib.sc2_jpeg_image_workspace_bytes(B, C, H, W)
    ws = _arena(ws_bytes, dev)
    ws[GUARD:GUARD + ws_bytes] = ws_fill
    at = lambda t: ctypes.c_void_p(t.data_ptr() + GUARD)      # noqa: E731
    assert (recon.data_ptr() + GUARD) % 4 == 0
    rc = lib.sc2_jpeg_image_codec(ctypes.c_void_p(x.data_ptr()), *x.stride(), B, C, H, W, quality, at(recon), at(sizes),
                                  at(coded) if want_bytes else ctypes.c_void_p(0), slot if want_bytes else 0, at(ws), ws_bytes,
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, S.hip.last_error()
    torch.cuda.synchronize()
    for arena, n in ((recon, x.numel()), (sizes, 4 * B), (coded, B * slot), (ws, ws_bytes)):
        assert bool((arena[:GUARD] == SENTINEL).all()) and bool((arena[GUARD + n:] == SENTINEL).all()), 'a guard byte was written'
    return (recon[GUARD:GUARD + x.numel()].reshape(x.shape).cpu(), sizes[GUARD:GUARD + 4 * B].view(torch.int32).cpu(),
            coded[GUARD:GUARD + B * slot].reshape(B, slot).cpu())


@pytest.mark.parametrize('C,H,W,quality', [(3, 47, 49, 100), (3, 13, 16 * IC.CHUNKED_MCUS - 5, 50), (1, 150, 130, 90)])
def test_outputs_stay_inside_their_arrays_and_nothing_depends_on_the_workspace(S, dev, C, H, W, quality):
    arrs = [IC.pixels(C, H, W, 'noise', seed=0), IC.pixels(C, H, W, 'gradient', seed=1)]
    x = torch.from_numpy(np.stack(arrs)).to(dev)
    header = S.hip.JPEG_HEADER_BYTES[S.hip.JPEG_RGB if C == 3 else S.hip.JPEG_GREY]
    runs = [_raw(S, x, quality, True, 0xFF), _raw(S, x, quality, True, 0x00), _raw(S, x, quality, True, 0x00)]
    for recon, sizes, slots in runs:
        for b, arr in enumerate(arrs):
            segment, _, decoded, size = IC.reference(arr, quality)
            assert int(sizes[b]) == size and torch.equal(recon[b], torch.from_numpy(decoded))
            n = size - header - 2
            assert slots[b, :n].numpy().tobytes() == segment
            assert bool((slots[b, n:] == SENTINEL).all()), 'bytes behind the segment were written'
    for other in runs[1:]:       # a workspace of ones, of zeros, and the same call again: bit-equal
        assert all(torch.equal(p, q) for p, q in zip(runs[0], other))
    recon, sizes, slots = _raw(S, x, quality, False, 0xFF)
    assert bool((slots == SENTINEL).all()), 'bytes were stored without a byte buffer'
    assert torch.equal(recon, runs[0][0]) and torch.equal(sizes, runs[0][1])


def test_refusals_launch_nothing(S, dev):
    hip, top = S.hip, S.hip.JPEG_IMAGE_MAX_SIDE
    x = torch.zeros(1, 3, 8, 8, dtype=torch.uint8, device=dev)
    with pytest.raises(hip.Sc2Error, match='no CPU fallback'):
        hip.jpeg_image_codec(x.cpu(), 90)
    with pytest.raises(hip.Sc2Error, match='uint8'):
        hip.jpeg_image_codec(x.float(), 90)
    with pytest.raises(hip.Sc2Error, match='channels'):
        hip.jpeg_image_codec(x[:, :2], 90)
    with pytest.raises(hip.Sc2Error, match=r'\[B,C,H,W\]'):
        hip.jpeg_image_codec(x[0], 90)
    for shape in ((1, 1, top + 1, 2), (1, 3, 2, top + 1)):
        with pytest.raises(hip.Sc2Error, match='at most {}'.format(top)):
            hip.jpeg_image_codec(torch.zeros(shape, dtype=torch.uint8, device=dev), 90)
    for quality in (0, 101, -1, 90.0, True):
        with pytest.raises(hip.Sc2Error, match=r'quality .*1\.\.100'):
            hip.jpeg_image_codec(x, quality)
    # the library's own checks, on outputs that must stay untouched
    lib = hip.lib()
    recon, sizes, ws = _arena(192, dev), _arena(4, dev), _arena(4096, dev)
    slot = hip.jpeg_image_max_bytes(3, 8, 8)
    coded = _arena(slot, dev)
    at = lambda t: ctypes.c_void_p(t.data_ptr() + GUARD)      # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(C=3, H=8, W=8, quality=90, slot_bytes=slot, ws_bytes=4096):
        return lib.sc2_jpeg_image_codec(ctypes.c_void_p(x.data_ptr()), 192, 64, 8, 1, 1, C, H, W, quality, at(recon), at(sizes), at(coded), slot_bytes,
                                        at(ws), ws_bytes, stream)
    unsupported, invalid = -2, -1
    assert [call(C=2), call(C=4), call(H=0), call(W=top + 1), call(quality=0), call(quality=101)] == [unsupported] * 6
    need = lib.sc2_jpeg_image_workspace_bytes(1, 3, 8, 8)
    assert [call(ws_bytes=need - 1), call(slot_bytes=slot - 1)] == [invalid] * 2
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (recon, sizes, ws, coded))
    assert call(ws_bytes=need) == 0
    torch.cuda.synchronize()
    assert int(sizes[GUARD:GUARD + 4].view(torch.int32)[0]) > hip.JPEG_HEADER_BYTES[hip.JPEG_RGB]


def _image(arr):
    from PIL import Image
    return Image.fromarray(arr[0] if arr.shape[0] == 1 else np.ascontiguousarray(arr.transpose(1, 2, 0)))


def _pixels_of(decoded):
    """forward_batch's `decoded` (a uint8 device tensor, or a list of PIL images) -> uint8 [B,C,H,W] on the host"""
    if isinstance(decoded, torch.Tensor):
        return decoded.cpu()
    arrs = [np.asarray(d) for d in decoded]
    return torch.from_numpy(np.stack([a[None] if a.ndim == 2 else a.transpose(2, 0, 1) for a in arrs]))


def test_module_equals_the_host_path(S, dev, monkeypatch):
    pytest.importorskip('PIL')
    calls = []
    kernel = S.hip.jpeg_image_codec
    monkeypatch.setattr(S.hip, 'jpeg_image_codec', lambda *a, **k: calls.append(1) or kernel(*a, **k))
    for (C, H, W), kwargs in (((3, 97, 131), dict(format='JPEG', quality=90)), ((1, 100, 75), dict(format='jpeg'))):
        m = S.PILImageModule(returns_file_size=True, **kwargs)
        images = [_image(IC.pixels(C, H, W, content, seed=s)) for s, content in enumerate(('gradient', 'noise', 'gradient'))]
        out = []
        for on in (False, True):
            monkeypatch.setattr(S.hip.host_policy, 'jpeg_image_hip', on)
            before = len(calls)
            decoded, sizes = m.forward_batch(images, dev)
            assert len(calls) - before == int(on) and isinstance(decoded, torch.Tensor) is on
            assert sizes == [m(img)[1] for img in images] and all(isinstance(n, int) for n in sizes)
            out.append((_pixels_of(decoded), sizes))
        assert torch.equal(out[0][0], out[1][0]) and out[0][1] == out[1][1]


def test_module_keeps_other_lists_on_the_host_path(S, dev, monkeypatch):
    """mixed sizes, a commented image, `optimize`: never the kernel, switch on or not, and the results agree."""
    pytest.importorskip('PIL')
    def refuse(*a, **k):
        raise AssertionError('the kernel was called')
    monkeypatch.setattr(S.hip, 'jpeg_image_codec', refuse)
    commented = _image(IC.pixels(3, 24, 40, 'gradient', seed=1))
    commented.info['comment'] = b'kept by convert, resize and crop'
    plain = dict(format='JPEG', quality=90)
    for images, kwargs in (([_image(IC.pixels(3, 24, 40, 'gradient')), _image(IC.pixels(3, 17, 33, 'noise'))], plain),
                           ([_image(IC.pixels(3, 24, 40, 'gradient')), commented], plain),
                           ([_image(IC.pixels(3, 24, 40, 'gradient'))], dict(format='JPEG', quality=90, optimize=True))):
        m = S.PILImageModule(returns_file_size=True, **kwargs)
        out = []
        for on in (False, True):
            monkeypatch.setattr(S.hip.host_policy, 'jpeg_image_hip', on)
            decoded, sizes = m.forward_batch(images, dev)
            assert isinstance(decoded, list) and sizes == [m(img)[1] for img in images]
            out.append(([np.asarray(d).copy() for d in decoded], sizes))
        assert all((p == q).all() for p, q in zip(out[0][0], out[1][0])) and out[0][1] == out[1][1]


class _StubClassifier(torch.nn.Module):
    """(the wrapper joins the samples of a batch along dim 1, as the reference does: B x 3 channels in)"""

    def __init__(self, B):
        super().__init__()
        self.conv = torch.nn.Conv2d(3 * B, 8, 3, padding=1)
        self.pool = torch.nn.AdaptiveAvgPool2d(1)
        self.fc = torch.nn.Linear(8, 10)

    def forward(self, x):
        return self.fc(torch.flatten(self.pool(torch.nn.functional.softplus(self.conv(x))), 1))


@pytest.mark.parametrize('B', [1, 3])
def test_input_compression_classifier_switch_on_and_off(S, dev, monkeypatch, B):
    pytest.importorskip('PIL')
    T = S.transforms
    torch.manual_seed(B)
    codec = T.Compose([S.PILImageModule(returns_file_size=True, format='JPEG', quality=90)])
    post = T.Compose([T.ToTensor(), T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])])
    model = S.CodecInputCompressionClassifier(_StubClassifier(B), dev, codec_encoder_decoder=codec, post_transform=post,
                                              analysis_config={'analyzer_configs': [{'key': 'FileSizeAccumulator', 'kwargs': {'unit': 'B'}}]}).to(dev).eval()
    model.activate_analysis()
    images = [_image(IC.pixels(3, 56, 72, content, seed=s)) for s, content in zip(range(B), ('gradient', 'noise', 'gradient'))]
    calls = []
    kernel = S.hip.jpeg_image_codec
    monkeypatch.setattr(S.hip, 'jpeg_image_codec', lambda *a, **k: calls.append(1) or kernel(*a, **k))
    results = []
    for on in (False, True):
        monkeypatch.setattr(S.hip.host_policy, 'jpeg_image_hip', on)
        model.clear_analysis()
        with torch.inference_mode():
            inputs = model._through_codec(images)
            logits = model(images)
        results.append((inputs.clone(), logits.clone(), list(model.analyzers[0].file_size_list)))
    assert len(calls) == 2                                        # two batches with the switch on, none with it off
    assert results[0][0].shape == (1, 3 * B, 56, 72) and results[0][1].shape == (1, 10) and len(results[0][2]) == 2 * B
    assert torch.equal(results[0][0], results[1][0]), 'the classifier inputs differ'
    assert torch.equal(results[0][1], results[1][1])
    assert results[0][2] == results[1][2]


def test_a_pil_first_post_transform_keeps_the_loop(S, dev, monkeypatch):
    """`Resize` + `ToTensor` + `Normalize` (and a callable of the caller's) work on the reopened PIL image: with the switch on the
    wrapper decides before any launch, the kernel is not called, and the result is the loop form's."""
    pytest.importorskip('PIL')
    T = S.transforms

    def refuse(*a, **k):
        raise AssertionError('the kernel was called')
    monkeypatch.setattr(S.hip, 'jpeg_image_codec', refuse)
    module = S.PILImageModule(returns_file_size=True, format='JPEG', quality=90)
    images = [_image(IC.pixels(3, 56, 72, content, seed=s)) for s, content in enumerate(('gradient', 'noise'))]
    normalize = T.Normalize([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    for post in (T.Compose([T.Resize(40), T.ToTensor(), normalize]), T.Compose([T.CenterCrop(32), T.ToTensor()]),
                 lambda img: T.to_tensor(img.convert('L'))):
        model = S.CodecInputCompressionClassifier(torch.nn.Identity(), dev, codec_encoder_decoder=T.Compose([module]), post_transform=post).eval()
        loop_model = S.CodecInputCompressionClassifier(torch.nn.Identity(), dev, codec_encoder_decoder=lambda img: module(img), post_transform=post).eval()
        out = []
        for on in (False, True):
            monkeypatch.setattr(S.hip.host_policy, 'jpeg_image_hip', on)
            out.append((model(images), loop_model(images)))
        assert out[0][0].is_cuda and all(torch.equal(out[0][1], t) for pair in out for t in pair)


def test_unit_table_and_normalize_equal_the_host_at_every_pixel_value(S, dev):
    """all 256 values in each of three channels: `to_tensor` of uint8 pixels on the device (a table built on the host) and `Normalize`
    behind it give the host's bits; the device's own division by the scalar 255 is what the table is there to avoid"""
    T = S.transforms
    every = torch.arange(256, dtype=torch.uint8).reshape(1, 16, 16).repeat(3, 1, 1)
    host = T.to_tensor(every)
    assert torch.equal(host, every.to(torch.float32) / 255)
    assert torch.equal(T.to_tensor(every.to(dev)).cpu(), host)
    assert torch.equal(T.to_tensor(torch.stack([every, every.flip(0)]).to(dev)).cpu(), torch.stack([host, host.flip(0)]))
    for mean, std in (([0.485, 0.456, 0.406], [0.229, 0.224, 0.225]), ([0.5, 0.5, 0.5], [0.5, 0.25, 0.3])):
        post = T.Compose([T.ToTensor(), T.Normalize(mean, std)])
        assert torch.equal(post(every.to(dev)).cpu(), post(every)), (mean, std)


def test_workspace_is_kept_per_device_stream_and_size(S, dev, monkeypatch):
    hip = S.hip
    monkeypatch.setattr(hip, '_jpeg_image_ws', dict())
    a = hip._jpeg_image_workspace(dev, 1024)
    assert a.dtype == torch.uint8 and a.numel() == 1024 and a.device == dev
    assert hip._jpeg_image_workspace(dev, 1024) is a                      # the same call again: the same buffer
    assert hip._jpeg_image_workspace(dev, 2048) is not a
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):                                         # another stream never shares a buffer with this one
        assert hip._jpeg_image_workspace(dev, 1024) is not a
    for n in range(hip._JPEG_IMAGE_WS_KEPT + 2):                          # only the most recent sizes are kept
        hip._jpeg_image_workspace(dev, 4096 + 256 * n)
    assert len(hip._jpeg_image_ws) == hip._JPEG_IMAGE_WS_KEPT
    assert hip._jpeg_image_workspace(dev, 1024) is not a
    x = torch.zeros(2, 3, 24, 40, dtype=torch.uint8, device=dev)
    hip.jpeg_image_codec(x, 90)
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream, hip.lib().sc2_jpeg_image_workspace_bytes(2, 3, 24, 40))
    assert key in hip._jpeg_image_ws
