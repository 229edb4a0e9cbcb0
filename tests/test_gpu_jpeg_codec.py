"""GPU: sc2_jpeg_tensor_codec (csrc/jpeg.hip) against the sequential integer restatement tests/ref_jpeg.py with NO tolerance -- the
bytes of every entropy-coded segment, the size of the file around it, the bits of low / high and the bits of the reconstruction -- and the module and
wrapper that call it against the host path they replace (Pillow per channel group)."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_cases as JC
import ref_jpeg as RJ

pytestmark = pytest.mark.gpu

GUARD = 64                      # sentinel elements in front of and behind every output
I32_SENTINEL = 0x5A5A5A5A
BYTE_SENTINEL = 0xA5
_REF = {}                       # (case key) -> reference results, computed once and shared


def _bits(t):
    return t.contiguous().view(torch.int32)


def _arena(n, dtype, fill, dev):
    return torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)


def _guards_intact(arena, n, fill):
    head, tail = arena[:GUARD], arena[GUARD + n:]
    if arena.dtype.is_floating_point:
        return bool(torch.isnan(head).all()) and bool(torch.isnan(tail).all())
    return bool((head == fill).all()) and bool((tail == fill).all())


def _launch(S, x, quality, want_bytes):
    """The raw entry on outputs that sit inside sentinel arenas.  -> dict of host arrays; asserts that nothing outside was written."""
    hip = S.hip
    B, C, H, W = x.shape
    n_img = B * (C // 3 + C % 3)
    dev = x.device
    recon = _arena(x.numel(), torch.float32, float('nan'), dev)
    sizes = _arena(n_img, torch.int32, I32_SENTINEL, dev)
    status = _arena(n_img, torch.int32, I32_SENTINEL, dev)
    extrema = _arena(2 * n_img, torch.float32, float('nan'), dev)
    slot = hip.jpeg_max_bytes(hip.JPEG_RGB if C >= 3 else hip.JPEG_GREY, H, W)
    coded = _arena(n_img * slot, torch.uint8, BYTE_SENTINEL, dev)
    e = lambda t: ctypes.c_void_p(t.data_ptr() + GUARD * t.element_size())      # noqa: E731
    rc = hip.lib().sc2_jpeg_tensor_codec(ctypes.c_void_p(x.data_ptr()), B, C, H, W, quality, e(recon), e(sizes), e(extrema), e(status),
                                         e(coded) if want_bytes else ctypes.c_void_p(0), slot if want_bytes else 0,
                                         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, hip.last_error()
    torch.cuda.synchronize()
    assert _guards_intact(recon, x.numel(), None) and _guards_intact(extrema, 2 * n_img, None)
    assert _guards_intact(sizes, n_img, I32_SENTINEL) and _guards_intact(status, n_img, I32_SENTINEL)
    assert _guards_intact(coded, n_img * slot, BYTE_SENTINEL)
    body = coded[GUARD:GUARD + n_img * slot].reshape(n_img, slot).cpu().numpy()
    if not want_bytes:
        assert (body == BYTE_SENTINEL).all(), 'bytes were stored without a byte buffer'
    return {'recon': recon[GUARD:GUARD + x.numel()].reshape(x.shape).cpu(), 'sizes': sizes[GUARD:GUARD + n_img].cpu().numpy(),
            'status': status[GUARD:GUARD + n_img].cpu().numpy(), 'extrema': extrema[GUARD:GUARD + 2 * n_img].reshape(n_img, 2).cpu(),
            'bytes': body}


def _reference(key, x_np, quality):
    if key not in _REF:
        _REF[key] = [RJ.tensor_codec(sample, quality) for sample in x_np]
    return _REF[key]


def _check_against_reference(out, ref, x_np, with_bytes):
    B, C = x_np.shape[:2]
    n = C // 3 + C % 3
    for b in range(B):
        recon, segments, extrema, status = ref[b]
        assert out['status'][b * n:(b + 1) * n].tolist() == status
        for g, (c0, nch) in enumerate(RJ.channel_groups(C)):
            i = b * n + g
            if status[g]:
                assert out['sizes'][i] == 0
                assert (out['bytes'][i] == BYTE_SENTINEL).all()
                assert bool(torch.isnan(out['recon'][b, c0:c0 + nch]).all()), 'a refused group was written'
                continue
            file_bytes = len(RJ.header('RGB' if nch == 3 else 'L', x_np.shape[2], x_np.shape[3], 50)) + len(segments[g]) + 2
            assert out['sizes'][i] == file_bytes, (b, g, out['sizes'][i], file_bytes)
            want = torch.tensor([float(extrema[g][0]), float(extrema[g][1])], dtype=torch.float32)
            assert torch.equal(_bits(out['extrema'][i]), _bits(want))
            if with_bytes:
                got = out['bytes'][i]
                assert got[:len(segments[g])].tobytes() == segments[g], (b, g)
                assert (got[len(segments[g]):] == BYTE_SENTINEL).all()
            assert torch.equal(_bits(out['recon'][b, c0:c0 + nch]), _bits(torch.from_numpy(recon[c0:c0 + nch]))), (b, g)


def _batch(C, B, H, W, shift):
    """B samples of different contents"""
    return np.stack([JC.features(JC.CONTENTS[(shift + b) % len(JC.CONTENTS)], C, H, W, seed=shift + b) for b in range(B)])


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C', [1, 2, 3, 5, 6])
def test_kernel_matches_the_reference(S, dev, C, B):
    """Every shape of the list, the qualities and contents rotating through it so that each (C, B) meets all of them; with the byte
    buffer and without; two launches bit-equal."""
    shapes = JC.GREY_SHAPES + JC.RGB_SHAPES
    for k, (H, W) in enumerate(shapes):
        shift = k + C + 2 * B
        quality = JC.QUALITIES[shift % len(JC.QUALITIES)]
        x_np = _batch(C, B, H, W, shift)
        ref = _reference((C, B, H, W, shift), x_np, quality)
        x = torch.from_numpy(x_np).to(dev)
        with_bytes = _launch(S, x, quality, True)
        _check_against_reference(with_bytes, ref, x_np, True)
        without = _launch(S, x, quality, False)
        _check_against_reference(without, ref, x_np, False)
        again = _launch(S, x, quality, True)
        for name in ('recon', 'extrema'):
            assert torch.equal(_bits(with_bytes[name]), _bits(again[name])) and torch.equal(_bits(with_bytes[name]), _bits(without[name]))
        assert (with_bytes['sizes'] == again['sizes']).all() and (with_bytes['bytes'] == again['bytes']).all()


@pytest.mark.parametrize('B', [1, 3])
def test_kernel_at_the_config_shape(S, dev, B):
    """[B,512,28,28] at quality 90: 172 images per sample (170 RGB, 2 grey), ReLU-like features."""
    rng = np.random.RandomState(7 + B)
    x_np = np.maximum(rng.randn(B, 512, 28, 28), 0).astype(np.float32) * 2 + np.float32(0.01) * rng.rand(B, 512, 1, 1).astype(np.float32)
    ref = _reference(('cfg', B), x_np, 90)
    x = torch.from_numpy(x_np).to(dev)
    _check_against_reference(_launch(S, x, 90, True), ref, x_np, True)
    res = S.hip.jpeg_tensor_codec(x, 90)
    assert res.bytes is None and res.sizes.shape == (B * 172,) and not bool(res.status.any())
    assert res.sizes.cpu().tolist() == [len(s) + 2 + S.hip.JPEG_HEADER_BYTES[S.hip.JPEG_RGB if g < 170 else S.hip.JPEG_GREY]
                                        for b in range(B) for g, s in enumerate(ref[b][1])]
    assert torch.equal(_bits(res.recon.cpu()), _bits(torch.from_numpy(np.stack([r[0] for r in ref]))))
    res_b = S.hip.jpeg_tensor_codec(x, 90, want_bytes=True)
    assert res_b.bytes.shape == (B * 172, S.hip.jpeg_max_bytes(S.hip.JPEG_RGB, 28, 28))
    assert bytes(res_b.bytes[0, :int(res_b.sizes[0]) - 625].cpu().numpy()) == ref[0][1][0]


def _with_bad_groups():
    """[3,7,12,20]: sample 0 clean; sample 1 with a negative minimum in group 1 and an all-zero grey group; sample 2 with a NaN in group 0
    and an infinity in group 1"""
    x = _batch(7, 3, 12, 20, 1)
    x[1, 4, 3, 5] = -0.5
    x[1, 6] = 0.0
    x[2, 1, 0, 0] = np.nan
    x[2, 3, 11, 19] = np.inf
    return x


def test_refused_groups_set_their_status_bit(S, dev):
    x_np = _with_bad_groups()
    ref = _reference('bad', x_np, 75)
    assert ref[1][3] == [0, RJ.STATUS_NEGATIVE_MIN, RJ.STATUS_ZERO_MAX] and ref[2][3] == [RJ.STATUS_NOT_FINITE, RJ.STATUS_NOT_FINITE, 0]
    assert (RJ.STATUS_NEGATIVE_MIN, RJ.STATUS_ZERO_MAX, RJ.STATUS_NOT_FINITE) == (S.hip.JPEG_NEGATIVE_MIN, S.hip.JPEG_ZERO_MAX, S.hip.JPEG_NOT_FINITE)
    x = torch.from_numpy(x_np).to(dev)
    _check_against_reference(_launch(S, x, 75, True), ref, x_np, True)
    _check_against_reference(_launch(S, x, 75, False), ref, x_np, False)


def _module_both_ways(S, monkeypatch, x, **kwargs):
    """PILTensorModule.forward per sample and forward_batch, switch off and on -> ((features, sizes) off, (features, sizes) on)"""
    m = S.PILTensorModule(returns_file_size=True, **kwargs)
    out = []
    for on in (False, True):
        monkeypatch.setattr(S.hip.host_policy, 'jpeg_codec_hip', on)
        single = [m(sample) for sample in x]
        feats, sizes = m.forward_batch(x)
        assert torch.equal(_bits(feats), _bits(torch.stack([f for f, _ in single]))) and sizes == [s for _, s in single]
        out.append((feats, sizes))
    return out


def test_module_equals_the_host_path(S, dev, monkeypatch):
    pytest.importorskip('PIL')
    for shape, kwargs in (((2, 512, 28, 28), dict(format='JPEG', quality=90)), ((3, 5, 13, 21), dict(format='jpeg')),
                          ((1, 8, 56, 56), dict(format='JPEG', quality=50)), ((2, 4, 7, 7), dict(format='JPEG', quality=100))):
        torch.manual_seed(shape[1])
        x = (torch.randn(shape).clamp_min(0) * 2 + 0.01 * torch.rand(shape[0], shape[1], 1, 1)).to(dev)
        (f_off, s_off), (f_on, s_on) = _module_both_ways(S, monkeypatch, x, **kwargs)
        assert torch.equal(_bits(f_off), _bits(f_on)), shape
        assert s_off == s_on, (shape, s_off, s_on)


def test_module_runs_a_refused_sample_on_the_host_path(S, dev, monkeypatch):
    pytest.importorskip('PIL')
    x = torch.from_numpy(_with_bad_groups()).to(dev)
    (f_off, s_off), (f_on, s_on) = _module_both_ways(S, monkeypatch, x, format='JPEG', quality=75)
    assert torch.equal(_bits(f_off), _bits(f_on)) and s_off == s_on


def test_binding_refusals(S, dev):
    x = torch.rand(1, 3, 8, 8, device=dev)
    with pytest.raises(S.hip.Sc2Error, match='no CPU fallback'):
        S.hip.jpeg_tensor_codec(x.cpu(), 90)
    with pytest.raises(S.hip.Sc2Error, match='f32'):
        S.hip.jpeg_tensor_codec(x.half(), 90)
    for shape in ((1, 3, 65, 8), (1, 3, 8, 65)):
        with pytest.raises(S.hip.Sc2Error, match='at most 64'):
            S.hip.jpeg_tensor_codec(torch.rand(shape, device=dev), 90)
    for quality in (0, 101, -1, 90.0, True):
        with pytest.raises(S.hip.Sc2Error, match='quality'):
            S.hip.jpeg_tensor_codec(x, quality)
    assert S.hip.jpeg_max_bytes(S.hip.JPEG_RGB, 64, 64) == RJ.max_bytes('RGB', 64, 64)
    assert S.hip.jpeg_max_bytes(S.hip.JPEG_GREY, 13, 21) == RJ.max_bytes('L', 13, 21)
    with pytest.raises(S.hip.Sc2Error):
        S.hip.jpeg_max_bytes(S.hip.JPEG_RGB, 65, 8)


def test_other_inputs_take_the_existing_path(S, dev, monkeypatch):
    """65 x 28, WEBP and `optimize` never reach the kernel, switch on or not."""
    pytest.importorskip('PIL')
    from PIL import features
    monkeypatch.setattr(S.hip.host_policy, 'jpeg_codec_hip', True)

    def refuse(*a, **k):
        raise AssertionError('the kernel was called')
    monkeypatch.setattr(S.hip, 'jpeg_tensor_codec', refuse)
    torch.manual_seed(3)
    cases = [((4, 65, 28), dict(format='JPEG', quality=90)), ((4, 16, 16), dict(format='JPEG', quality=90, optimize=True)),
             ((4, 16, 16), dict(format='JPEG', quality=90, subsampling=0))]
    if features.check('webp'):
        cases.append(((4, 16, 16), dict(format='WEBP', quality=90)))
    for shape, kwargs in cases:
        x = torch.rand(shape, device=dev) + 0.1
        m = S.PILTensorModule(returns_file_size=True, **kwargs)
        y, size = m(x)
        ys, sizes = m.forward_batch(x.unsqueeze(0))
        assert y.shape == x.shape and size > 0 and torch.equal(_bits(ys[0]), _bits(y)) and sizes == [size]


class _StubClassifier(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = torch.nn.Conv2d(3, 7, 3, padding=1)
        self.act = torch.nn.Softplus()
        self.layer2 = torch.nn.Conv2d(21, 8, 3, padding=1)      # (the wrapper joins the samples of a batch along dim 1: 3 x 7 channels)
        self.avgpool = torch.nn.AdaptiveAvgPool2d(1)
        self.fc = torch.nn.Linear(8, 10)


def test_feature_compression_classifier_switch_on_and_off(S, dev, monkeypatch):
    pytest.importorskip('PIL')
    torch.manual_seed(0)
    codec = S.transforms.Compose([S.PILTensorModule(returns_file_size=True, format='JPEG', quality=90)])
    model = S.CodecFeatureCompressionClassifier(
        _StubClassifier(), dev, encoder_config={'sequential': ['conv1', 'act']}, codec_encoder_decoder=codec,
        decoder_config={'sequential': ['layer2', 'avgpool']}, classifier_config={'sequential': ['fc']},
        analysis_config={'analyzer_configs': [{'key': 'FileSizeAccumulator', 'kwargs': {'unit': 'B'}}]}).to(dev).eval()
    model.activate_analysis()
    x = torch.rand(3, 3, 20, 28, device=dev)
    results = []
    for on in (False, True):
        monkeypatch.setattr(S.hip.host_policy, 'jpeg_codec_hip', on)
        model.clear_analysis()
        with torch.inference_mode():
            logits = model(x)
        results.append((logits.clone(), list(model.analyzers[0].file_size_list)))
    assert results[0][0].shape == (1, 10) and len(results[0][1]) == 3
    assert torch.equal(_bits(results[0][0]), _bits(results[1][0]))
    assert results[0][1] == results[1][1]
