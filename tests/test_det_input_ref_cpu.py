"""CPU: the restatement of sc2_det_input (tests/ref_det_input.py) against exact-weight float64, the host chain (to_tensor, normalise,
F.interpolate with a recomputed scale factor) against the same float64, both within the derived bound `delta`, and the 3 x 256 table
against the host's normalised values bit for bit."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_det_input as RI  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
ODD_MEAN, ODD_STD = [0.1, 0.5, 0.9], [0.3, 1.7, 0.05]
# (h, w) -> (oh, ow): up, down, scale 1, one-pixel sides, the detector's own sizes
SHAPES = [((1, 7), (1, 7)), ((7, 1), (14, 2)), ((37, 53), (37, 53)), ((53, 37), (133, 93)), ((200, 120), (80, 48)),
          ((3, 667), (6, 1334)), ((480, 640), (800, 1066)), ((100, 1000), (133, 1333))]


def _source(h, w, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3), dtype=np.uint8)


def _host_chain(S, src, oh, ow, flip, mean, std):
    """to_tensor -> [flip] -> the transform's normalise -> F.interpolate(scale_factor, recompute_scale_factor=True)"""
    from sc2bench_amd import detection, transforms
    h, w, _ = src.shape
    image = transforms.to_tensor(src)
    if flip:
        image = image.flip(-1)
    image = detection.GeneralizedRCNNTransform(oh, ow, mean, std).normalize(image)
    # a scale factor that floors to (oh, ow), as the transform's own min(min_size / min, max_size / max) does for its sizes
    scale = [(oh + 0.5) / h, (ow + 0.5) / w]
    out = F.interpolate(image[None], scale_factor=scale, mode='bilinear', recompute_scale_factor=True, align_corners=False)[0]
    assert tuple(out.shape[-2:]) == (oh, ow)
    return out.numpy()


@pytest.mark.parametrize('mean,std', [(MEAN, STD), (ODD_MEAN, ODD_STD)])
def test_table_equals_the_hosts_normalised_values_bit_for_bit(S, mean, std):
    from sc2bench_amd import detection, transforms
    pixels = np.arange(256, dtype=np.uint8).reshape(16, 16)
    image = transforms.to_tensor(np.stack([pixels] * 3, axis=2))
    want = detection.GeneralizedRCNNTransform(16, 16, mean, std).normalize(image).numpy().reshape(3, 256)
    got = RI.table_f32(mean, std)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.abs(got - RI.table_f64(mean, std)).max() <= 2.0 ** -23 * np.abs(got).max()


@pytest.mark.parametrize('src_hw,out_hw', SHAPES)
def test_f32_restatement_and_host_chain_stay_within_delta_of_float64(S, src_hw, out_hw):
    (h, w), (oh, ow) = src_hw, out_hw
    for flip, (mean, std) in ((False, (MEAN, STD)), (True, (ODD_MEAN, ODD_STD))):
        src = _source(h, w, seed=h * 1000 + w)
        exact = RI.det_input_f64(src, oh, ow, flip, mean, std)
        bound = RI.delta(h, w, mean, std)
        f32 = RI.det_input_f32(src, oh, ow, flip, mean, std)
        assert f32.dtype == np.float32 and f32.shape == (3, oh, ow)
        err32 = float(np.abs(f32.astype(np.float64) - exact).max())
        host = _host_chain(S, src, oh, ow, flip, mean, std)
        err_host = float(np.abs(host.astype(np.float64) - exact).max())
        print('{}x{} -> {}x{} flip {}: f32 {:.3e}, host chain {:.3e}, delta {:.3e}'.format(h, w, oh, ow, flip, err32, err_host, bound))
        assert err32 <= bound
        assert err_host <= bound


def test_scale_one_gives_the_table_values(S):
    src = _source(64, 64, seed=9)
    out = RI.det_input_f32(src, 64, 64, False, MEAN, STD)
    table = RI.table_f32(MEAN, STD)
    for c in range(3):
        assert np.array_equal(out[c], table[c][src[:, :, c]])
    flipped = RI.det_input_f32(src, 64, 64, True, MEAN, STD)
    assert np.array_equal(flipped, out[:, :, ::-1])


def test_delta_is_the_stated_formula():
    table = RI.table_f64(MEAN, STD)
    want = 2 * 2.0 ** -14 * (table.max() - table.min()) + 8 * 2.0 ** -24 * np.abs(table).max()      # spacing_f32(640) = 2^-14
    assert math.isclose(RI.delta(480, 640, MEAN, STD), want, rel_tol=1e-12)
