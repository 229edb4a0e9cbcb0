"""tests/ref_cls_input.py against Pillow itself, byte for byte: `img.crop(box).resize(...)` (the train form) and `Resize -> CenterCrop`
(the evaluation form) on random 8-bit images, and the trimmed stored box against the whole image."""
import numpy as np
import pytest

import ref_cls_input as RC

Image = pytest.importorskip('PIL.Image')


def source(h, w, seed=0):
    return np.random.RandomState(1000 * h + w + seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


# (image h, w), (top, left, ch, cw), (nh, nw)
CROPS = [
    pytest.param((20, 31), (3, 4, 5, 7), (12, 12), id='upscale-5x7-to-12x12'),
    pytest.param((20, 31), (2, 5, 12, 12), (12, 12), id='ratio-1-both'),
    pytest.param((20, 40), (4, 3, 12, 30), (12, 12), id='ratio-1-rows-2.5-columns'),
    pytest.param((33, 47), (1, 2, 30, 40), (12, 16), id='ratio-2.5'),
    pytest.param((41, 80), (0, 1, 39, 78), (10, 20), id='ratio-3.9'),
    pytest.param((50, 70), (2, 6, 48, 64), (12, 16), id='ratio-4-exactly'),
    pytest.param((12, 9), (0, 3, 9, 1), (12, 12), id='one-pixel-wide'),
    pytest.param((9, 12), (2, 0, 1, 9), (12, 8), id='one-pixel-high'),
    pytest.param((40, 60), (1, 3, 37, 53), (24, 40), id='non-square-output'),
    pytest.param((375, 500), (40, 61, 288, 301), (224, 224), id='imagenet-size'),
]


@pytest.mark.parametrize('hw, crop, out', CROPS)
@pytest.mark.parametrize('flip', [False, True])
def test_crop_then_resize_is_pillows(hw, crop, out, flip):
    image = source(*hw)
    top, left, ch, cw = crop
    nh, nw = out
    want = Image.fromarray(image).crop((left, top, left + cw, top + ch)).resize((nw, nh), Image.BILINEAR)
    if flip:
        want = want.transpose(Image.FLIP_LEFT_RIGHT)
    got, box, fields = RC.crop_resize(image, top, left, ch, cw, nh, nw, flip)
    assert box.shape == (ch, cw, 3) and (fields['full_h'], fields['full_w']) == (ch, cw)
    assert np.array_equal(got, np.asarray(want))


# (image h, w), Resize's size, (oh, ow)
EVALS = [
    pytest.param((101, 77), 48, (40, 40), id='101x77-resize-48-crop-40'),
    pytest.param((60, 48), 48, (40, 32), id='ratio-1-both'),
    pytest.param((120, 150), 48, (40, 56), id='ratio-2.5'),
    pytest.param((156, 200), 40, (32, 40), id='ratio-3.9'),
    pytest.param((160, 192), 40, (40, 40), id='ratio-4-exactly'),
    pytest.param((5, 7), 12, (12, 12), id='upscale'),
    pytest.param((1, 9), (8, 18), (6, 12), id='one-pixel-high'),
    pytest.param((9, 1), (18, 4), (10, 4), id='one-pixel-wide'),
    pytest.param((375, 500), 256, (224, 224), id='imagenet-size'),
]


@pytest.mark.parametrize('hw, size, out', EVALS)
def test_resize_then_center_crop_is_pillows_and_the_trimmed_box_gives_the_same_bytes(hw, size, out):
    image = source(*hw)
    oh, ow = out
    nh, nw = RC.resized_hw(hw[0], hw[1], size)
    top, left = RC.center_origin(nh, nw, oh, ow)
    want = Image.fromarray(image).resize((nw, nh), Image.BILINEAR).crop((left, top, left + ow, top + oh))
    whole, box_whole, _ = RC.resize_center_crop(image, size, oh, ow, trimmed=False)
    trimmed, box, fields = RC.resize_center_crop(image, size, oh, ow, trimmed=True)
    assert box_whole.shape == image.shape
    assert np.array_equal(whole, np.asarray(want))
    assert np.array_equal(trimmed, whole)
    assert box.shape[0] <= hw[0] and box.shape[1] <= hw[1]
    assert np.array_equal(box, image[fields['row0']:fields['row0'] + box.shape[0], fields['col0']:fields['col0'] + box.shape[1]])


def test_trimmed_box_is_smaller_at_the_imagenet_size_and_one_row_less_is_refused():
    image = source(375, 500)
    _, box, fields = RC.resize_center_crop(image, 256, 224, 224)
    share = box.shape[0] * box.shape[1] / (375 * 500)
    assert 0.56 < share < 0.60, share       # 224 / 256 of the rows, 224 / 341 of the columns, and the taps' margins
    r0, rh, c0, cw = RC.stored_box(500, 500, 256, 256, 16, 16, 224, 224)
    assert 0.76 < rh * cw / (500 * 500) < 0.79      # a square source: (224 / 256)^2 = 77 % and the margins
    assert RC.status(box.shape, oh=224, ow=224, **fields) == 0
    assert RC.status(box[1:].shape, oh=224, ow=224, **dict(fields, row0=fields['row0'] + 1)) == RC.TAP
    assert RC.status(box[:-1].shape, oh=224, ow=224, **fields) == RC.TAP
    assert RC.status(box[:, :-1].shape, oh=224, ow=224, **fields) == RC.TAP
    assert RC.status(box.shape, oh=224, ow=224, **dict(fields, full_h=1025)) == RC.RATIO      # 1025 > 4 * 256
    assert RC.status(box.shape, oh=224, ow=224, **dict(fields, nh=93)) == RC.BAD                # the window leaves the resized image


def test_identity_axis_reads_no_neighbour():
    """an axis of equal lengths: one coefficient of 2^22 -- Pillow's skipped pass -- so the box needs exactly the window's pixels"""
    bounds, k = RC.axis_coeffs(48, 48)
    assert bounds.tolist() == [[i, 1] for i in range(48)] and (k == 1 << 22).all()
    assert RC.stored_box(60, 48, 60, 48, 10, 8, 40, 32) == (10, 40, 8, 32)


def test_normalize_is_torchs():
    torch = pytest.importorskip('torch')
    u8 = source(9, 11)
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    x = torch.from_numpy(u8).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    want = (x - torch.tensor(mean).view(3, 1, 1)) / torch.tensor(std).view(3, 1, 1)
    assert torch.equal(torch.from_numpy(RC.normalize(u8, mean, std)), want)
