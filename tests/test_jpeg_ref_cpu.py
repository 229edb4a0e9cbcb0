"""CPU: the sequential integer restatement of baseline JPEG (tests/ref_jpeg.py) against Pillow's codec -- the file byte for byte, the
decoded image pixel for pixel -- and the restated tensor module against transforms.PILTensorModule on CPU tensors.  This is what
entitles tests/test_gpu_jpeg_codec.py to hold the kernel to the restatement with no tolerance."""
import io

import numpy as np
import pytest
import torch

import jpeg_cases as JC
import ref_jpeg as RJ

Image = pytest.importorskip('PIL.Image')


def _pillow(pixels, quality):
    """-> (file bytes, decoded uint8 array in the layout of `pixels`)"""
    rgb = pixels.ndim == 3
    img = Image.fromarray(np.ascontiguousarray(pixels.transpose(1, 2, 0)) if rgb else pixels, mode='RGB' if rgb else 'L')
    coded = io.BytesIO()
    img.save(coded, format='JPEG', quality=quality)
    back = np.array(Image.open(io.BytesIO(coded.getvalue())))
    return coded.getvalue(), back.transpose(2, 0, 1) if rgb else back


def _cases(channels, shapes):
    return [(channels, H, W, q) for (H, W) in shapes for q in JC.QUALITIES]


@pytest.mark.parametrize('channels,H,W,quality', _cases(1, JC.GREY_SHAPES) + _cases(3, JC.RGB_SHAPES))
def test_restatement_equals_pillow(channels, H, W, quality):
    for k, content in enumerate(JC.CONTENTS):
        pixels = JC.pixels(content, channels, H, W, seed=k + quality)
        theirs, decoded = _pillow(pixels, quality)
        segment, coefs = RJ.encode(pixels, quality)
        mode = 'RGB' if channels == 3 else 'L'
        assert RJ.header(mode, H, W, quality) + segment + b'\xff\xd9' == theirs, content
        assert RJ.file_bytes(pixels, quality) == theirs
        assert len(segment) <= RJ.max_bytes(mode, H, W)
        assert np.array_equal(RJ.decode(coefs), decoded), content


def test_isolated_content_has_runs_above_fifteen():
    """the ZRL symbol is exercised: the 'isolated' content leaves one high-frequency coefficient behind more than 15 zeros"""
    for channels, (H, W) in ((1, (28, 28)), (3, (40, 24))):
        _, coefs = RJ.encode(JC.pixels('isolated', channels, H, W, seed=0), 50)
        assert JC.longest_zero_run(coefs, RJ.ZIGZAG) > 15


def test_dummy_blocks_are_exercised():
    """W = 24 leaves a dummy luma column, H = 40 a dummy luma row: both in the list"""
    assert (40, 24) in JC.RGB_SHAPES and any(-(-W // 8) % 2 for _, W in JC.RGB_SHAPES) and any(-(-H // 8) % 2 for H, _ in JC.RGB_SHAPES)


def test_package_header_equals_the_restatement(S):
    from sc2bench_amd import jpeg_format
    for mode, H, W in (('L', 1, 1), ('L', 64, 40), ('RGB', 28, 28), ('RGB', 7, 35)):
        for quality in JC.QUALITIES:
            assert jpeg_format.header(mode, H, W, quality) == RJ.header(mode, H, W, quality)
            assert jpeg_format.checked_header_bytes(mode, H, W, quality) == len(RJ.header(mode, H, W, quality))


@pytest.mark.parametrize('C', [1, 2, 3, 4, 5, 8])
def test_restated_module_equals_pil_tensor_module(S, C):
    from sc2bench_amd.analysis import get_binary_object_size
    for (H, W), quality in (((13, 21), 90), ((28, 28), 75), ((7, 7), 50)):
        torch.manual_seed(C + H)
        x = torch.randn(C, H, W).abs() * 3 + 0.1
        kwargs = dict(format='JPEG') if quality == 75 else dict(format='JPEG', quality=quality)
        features, size = S.PILTensorModule(returns_file_size=True, **kwargs)(x)
        recon, segments, extrema, status = RJ.tensor_codec(x.numpy(), quality)
        assert status == [0] * len(segments)
        assert torch.equal(features.view(torch.int32), torch.from_numpy(recon).view(torch.int32))
        side_info = 2 * get_binary_object_size([torch.zeros(()) for _ in segments], unit_size=1)
        groups = RJ.channel_groups(C)
        assert size == RJ.file_size([(seg, n) for seg, (_, n) in zip(segments, groups)], H, W, quality, side_info)


def test_status_of_refused_groups():
    x = np.ones((3, 4, 4), dtype=np.float32)
    assert RJ.group_status(x) == 0
    neg, zero, nan, inf = x.copy(), np.zeros_like(x), x.copy(), x.copy()
    neg[1, 2, 3], nan[0, 0, 0], inf[2, 3, 3] = -1.0, np.nan, np.inf
    assert [RJ.group_status(v) for v in (neg, zero, nan, inf)] == [RJ.STATUS_NEGATIVE_MIN, RJ.STATUS_ZERO_MAX, RJ.STATUS_NOT_FINITE,
                                                                  RJ.STATUS_NOT_FINITE]
