"""CPU: tests/ref_rcnn_input.py (the float64 restatement of csrc/rcnn_input.hip) against hand-worked cases and against torch on the
host -- `F.interpolate(..., recompute_scale_factor=True).mul(255).byte()` for the resize rule, `(to_tensor(u8) - mean) / std` for the
normalise-and-pad reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ref_rcnn_input as RR

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
RESIZE_SHAPES = [((7, 5), (112, 80)), ((37, 53), (80, 114)), ((53, 37), (114, 80)), ((20, 97), (27, 133)), ((100, 120), (80, 96))]


def test_resize_ref_one_pixel():
    x = np.array([[[0.25]]])
    got = RR.resize_ref(x, 3, 2)
    assert got.shape == (1, 3, 2) and (got == 0.25 * 255.0).all()


def test_resize_ref_two_by_two_to_four_by_four():
    """scale 0.5: src = -0.25 -> 0, 0.25, 0.75, 1.25 -> weights (1, 0), (0.75, 0.25), (0.25, 0.75), (clamped neighbour: the last pixel)"""
    a, b, c, d = 0.0, 0.4, 0.8, 1.0
    x = np.array([[[a, b], [c, d]]])
    got = RR.resize_ref(x, 4, 4) / 255.0
    row = lambda p, q: np.array([p, 0.75 * p + 0.25 * q, 0.25 * p + 0.75 * q, q])      # noqa: E731
    top, bot = row(a, b), row(c, d)
    want = np.stack([top, 0.75 * top + 0.25 * bot, 0.25 * top + 0.75 * bot, bot])
    assert np.allclose(got[0], want, rtol=0, atol=1e-15)


def test_resize_ref_keeps_a_constant():
    got = RR.resize_ref(np.full((3, 13, 9), 0.6), 31, 17)
    assert np.abs(got - 0.6 * 255.0).max() < 1e-12


def test_rule_accepts_floor_and_the_margin_only():
    v = np.array([[[10.5, 11.99999, 12.00001, 13.5]]])
    delta = 1e-4
    assert RR.check_resize(np.array([[[10, 11, 12, 13]]]), v, delta) == (0, 0.0)
    wrong, share = RR.check_resize(np.array([[[10, 12, 11, 13]]]), v, delta)       # either side of 12, by the margin clause
    assert wrong == 0 and share == 0.5
    assert RR.check_resize(np.array([[[11, 11, 12, 13]]]), v, delta)[0] == 1       # 10.5 is nowhere near an integer
    assert RR.check_resize(np.array([[[10, 13, 12, 13]]]), v, delta)[0] == 1       # one above round() is never right
    assert RR.resize_delta(100, 640) == 255.0 * 2.0 * float(np.spacing(np.float32(640))) + 2e-4


@pytest.mark.parametrize('src,dst', RESIZE_SHAPES)
def test_torch_cpu_resize_meets_the_rule(src, dst):
    (H, W), (oh, ow) = src, dst
    x = torch.rand(3, H, W, generator=torch.Generator().manual_seed(H * 1000 + W))
    scale = min(80.0 / min(H, W), 133.0 / max(H, W))
    y = F.interpolate(x[None], scale_factor=scale, mode='bilinear', recompute_scale_factor=True, align_corners=False)[0]
    assert tuple(y.shape[-2:]) == (oh, ow)
    wrong, share = RR.check_resize(y.mul(255).byte().numpy(), RR.resize_ref(x.numpy(), oh, ow), RR.resize_delta(H, W))
    assert wrong == 0
    assert share <= RR.MARGIN_CAP


def test_normalize_pad_ref_is_torch_cpu_on_every_byte():
    from sc2bench_amd import transforms as T
    p = np.tile(np.arange(256, dtype=np.uint8).reshape(1, 16, 16), (3, 1, 1))
    got = RR.normalize_pad_ref(p, MEAN, STD, 32, 32)
    want = (T.to_tensor(torch.from_numpy(p)) - torch.tensor(MEAN)[:, None, None]) / torch.tensor(STD)[:, None, None]
    assert got.dtype == np.float32
    assert (got[:, :16, :16].view(np.uint32) == want.numpy().view(np.uint32)).all()
    pad = np.ones((3, 32, 32), dtype=bool)
    pad[:, :16, :16] = False
    assert (got.view(np.uint32)[pad] == 0).all()       # +0.0, not -0.0
