"""tests/ref_pil_resize.py against Pillow itself: the bilinear and the nearest resize of 8-bit images, byte for byte, over up- and
down-scaling and sources from 1 x 9 to 500 x 333.  The restatement is what the device kernel is tested against, so it has to BE Pillow."""
import numpy as np
import pytest
from PIL import Image

import ref_pil_resize as ref

SOURCES = [(1, 9), (7, 5), (33, 50), (64, 64), (281, 500), (375, 500), (500, 333)]       # (h, w)
SHORT_SIDES = [1, 3, 8, 64, 256, 300, 513, 700, 1026]


def _target(h, w, s):
    short, long_ = (w, h) if w <= h else (h, w)
    new_long = int(s * long_ / short)
    return (new_long, s) if w <= h else (s, new_long)        # (nh, nw)


# (each source also at its own short side: both passes skipped -- 54 + 7 = 61 cases)
CASES = [(h, w) + _target(h, w, s) for (h, w) in SOURCES for s in SHORT_SIDES + [min(h, w)] if 1 <= max(_target(h, w, s)) <= 1400]


def test_case_list():
    assert len(CASES) == 61
    assert any(nh > h for h, w, nh, nw in CASES) and any(nh < h for h, w, nh, nw in CASES) and any(nw == w for h, w, nh, nw in CASES)


@pytest.fixture(scope='module')
def sources():
    rng = np.random.RandomState(0)
    out = {}
    for h, w in SOURCES:
        mask = rng.randint(0, 22, (h, w)).astype(np.uint8)
        mask[mask == 21] = 255
        out[h, w] = rng.randint(0, 256, (h, w, 3)).astype(np.uint8), mask
    return out


@pytest.mark.parametrize('h,w,nh,nw', CASES)
def test_bilinear_and_nearest_equal_pillow(sources, h, w, nh, nw):
    image, mask = sources[h, w]
    want = np.asarray(Image.fromarray(image).resize((nw, nh), Image.BILINEAR))
    assert np.array_equal(ref.resize_bilinear(image, nh, nw), want)
    want = np.asarray(Image.fromarray(mask).resize((nw, nh), Image.NEAREST))
    assert np.array_equal(ref.resize_nearest(mask, nh, nw), want)


def test_hand_worked_coefficients():
    # 2 -> 4 (upscale, support 1): centers 0.25, 0.75, 1.25, 1.75; output 1 weighs the sources 0.75 : 0.25
    bounds, k = ref.coeffs(2, 4)
    assert bounds.tolist() == [[0, 1], [0, 2], [0, 2], [1, 1]]
    assert k[0, 0] == 1 << 22 and k[1, :2].tolist() == [3 << 20, 1 << 20] and k[2, :2].tolist() == [1 << 20, 3 << 20]
    # 4 -> 2 (downscale by 2, support 2): output 0 sees sources 0..2 with weights 0.75, 0.75, 0.25 -> 3/7, 3/7, 1/7
    bounds, k = ref.coeffs(4, 2)
    assert bounds.tolist() == [[0, 3], [1, 3]] and k.shape[1] == 5
    assert k[0, :3].tolist() == [int(0.5 + 3 / 7 * 2 ** 22), int(0.5 + 3 / 7 * 2 ** 22), int(0.5 + 1 / 7 * 2 ** 22)]
    # equal lengths: the one coefficient 2^22 (the pass Pillow skips)
    bounds, k = ref.coeffs(5, 5)
    assert bounds[:, 0].tolist() == [0, 1, 2, 3, 4] and (k[:, 0] == 1 << 22).all() and (k[:, 1:] == 0).all()
    assert ref.nearest_table(3, 7).tolist() == [0, 0, 1, 1, 1, 2, 2] and ref.nearest_table(7, 3).tolist() == [1, 3, 5]


def test_augment_equals_the_pillow_chain():
    import torch
    from sc2bench_amd import transforms as T
    rng = np.random.RandomState(3)
    image, mask = rng.randint(0, 256, (37, 50, 3)).astype(np.uint8), rng.randint(0, 21, (37, 50)).astype(np.uint8)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    for nh, nw, flip, top, left, out, pad_h, pad_w in ((74, 100, True, 41, 67, 33, 74, 100), (20, 27, False, 0, 0, 33, 33, 33),
                                                       (37, 50, True, 4, 17, 33, 37, 50), (24, 33, False, 0, 0, 33, 33, 33)):
        got = ref.augment(image, mask, nh, nw, flip, top, left, out, out, pad_h, pad_w, mean, std)
        want = T.DeferredSegSample(image, mask, nh, nw, flip, top, left, out, out, pad_h, pad_w, mean, std).host()
        assert torch.equal(torch.from_numpy(got[0]), want[0]) and torch.equal(torch.from_numpy(got[1]), want[1])
