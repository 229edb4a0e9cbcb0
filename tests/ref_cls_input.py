"""The two ImageNet input chains restated in numpy on tests/ref_pil_resize.py (which tests/test_pil_resize_ref_cpu.py proves against
Pillow): what csrc/cls_input.hip computes.  tests/test_cls_input_ref_cpu.py proves this file against Pillow itself, byte for byte.

A sample is a STORED BOX of a full image, resampled with the full image's coefficients, flipped, and shown through a window:
    crop_resize         `img.crop(box).resize((nw, nh), BILINEAR)`: the box is the crop, full = the crop's size (the train form)
    resize_center_crop  `Resize(size) -> CenterCrop((oh, ow))` of the whole image (the evaluation form)
    stored_box          the rows and columns of the full image that a window's taps read
    window              the general form, from a stored box and the twelve descriptor fields: the kernel's arithmetic
    normalize           ToTensor + Normalize in float32, as torch divides and subtracts
An axis of equal lengths is the pass Pillow skips: one coefficient of 2^22 on the pixel itself.
"""
import numpy as np

import ref_pil_resize as ref

RATIO, BAD, TAP = 1, 2, 3      # the kernel's status words


def axis_coeffs(n_in, n_out):
    """-> (bounds [n_out, 2], k [n_out, ksize]) of `ref_pil_resize.coeffs`, or the identity pass of an axis of equal lengths"""
    if n_in == n_out:
        bounds = np.stack([np.arange(n_out), np.ones(n_out, np.int64)], 1).astype(np.int64)
        return bounds, np.full((n_out, 1), 1 << ref.PRECISION_BITS, np.int64)
    return ref.coeffs(n_in, n_out)


def tap_span(n_in, n_out, origin, length):
    """[lo, hi): the source indices the resized positions origin .. origin + length - 1 read"""
    bounds, _ = axis_coeffs(n_in, n_out)
    first = bounds[origin:origin + length, 0]
    return int(first.min()), int((first + bounds[origin:origin + length, 1]).max())


def stored_box(full_h, full_w, nh, nw, top, left, oh, ow, flip=False):
    """-> (row0, h, col0, w): the smallest box of the full image that holds every tap of the oh x ow window at (top, left) of the
    resized, flipped image"""
    r0, r1 = tap_span(full_h, nh, top, oh)
    c0, c1 = tap_span(full_w, nw, nw - left - ow if flip else left, ow)
    return r0, r1 - r0, c0, c1 - c0


def resized_hw(h, w, size):
    """torchvision's `Resize` rule: int -> the short side becomes `size`, the long side int(size * long / short); (h, w) -> exact"""
    if isinstance(size, int):
        short, long_ = (w, h) if w <= h else (h, w)
        new_short, new_long = size, int(size * long_ / short)
        return (new_long, new_short) if w <= h else (new_short, new_long)
    return int(size[0]), int(size[1])


def center_origin(nh, nw, oh, ow):
    return int(round((nh - oh) / 2.0)), int(round((nw - ow) / 2.0))


def status(box_shape, full_h, full_w, row0, col0, nh, nw, flip, top, left, oh, ow):
    """the kernel's status word for a descriptor whose offset lies inside the buffer"""
    h, w = box_shape[:2]
    sides = all(1 <= v <= 16384 for v in (h, w, full_h, full_w, nh, nw))
    if not sides or row0 < 0 or col0 < 0 or row0 + h > full_h or col0 + w > full_w or top < 0 or left < 0 or top + oh > nh or \
            left + ow > nw or flip not in (0, 1, False, True):
        return BAD
    if full_h > 4 * nh or full_w > 4 * nw:
        return RATIO
    r0, rh, c0, cw = stored_box(full_h, full_w, nh, nw, top, left, oh, ow, flip)
    if r0 < row0 or r0 + rh > row0 + h or c0 < col0 or c0 + cw > col0 + w:
        return TAP
    return 0


def _pass(a, n_in, n_out, offset, indices):
    """resamples axis 1 of the uint8 [R, w, C] box `a`, which holds the source indices offset .. offset + w - 1 of an axis of length
    n_in, at the resized positions `indices` -> uint8 [R, len(indices), C]"""
    bounds, k = axis_coeffs(n_in, n_out)
    out = np.empty((a.shape[0], len(indices), a.shape[2]), np.uint8)
    for o, j in enumerate(indices):
        first, count = int(bounds[j, 0]), int(bounds[j, 1])
        lo = first - offset
        assert lo >= 0 and lo + count <= a.shape[1], 'a tap outside the stored box'
        acc = (1 << (ref.PRECISION_BITS - 1)) + (a[:, lo:lo + count, :].astype(np.int64) * k[j, :count][None, :, None]).sum(1)
        out[:, o, :] = np.clip(acc >> ref.PRECISION_BITS, 0, 255)
    return out


def window(box, full_h, full_w, row0, col0, nh, nw, flip, top, left, oh, ow):
    """uint8 [h, w, 3] stored box -> uint8 [oh, ow, 3]: the horizontal pass over the box's rows to 8 bits, then the vertical pass"""
    assert status(box.shape, full_h, full_w, row0, col0, nh, nw, flip, top, left, oh, ow) == 0
    cols = [nw - 1 - (left + x) if flip else left + x for x in range(ow)]
    a = _pass(box, full_w, nw, col0, cols)
    a = _pass(a.transpose(1, 0, 2), full_h, nh, row0, [top + y for y in range(oh)]).transpose(1, 0, 2)
    return np.ascontiguousarray(a)


def crop_resize(image, top, left, ch, cw, nh, nw, flip=False):
    """`img.crop((left, top, left + cw, top + ch)).resize((nw, nh), BILINEAR)` [flipped] -> (uint8 [nh, nw, 3], box, fields)"""
    box = np.ascontiguousarray(image[top:top + ch, left:left + cw])
    fields = dict(full_h=ch, full_w=cw, row0=0, col0=0, nh=nh, nw=nw, flip=bool(flip), top=0, left=0)
    return window(box, oh=nh, ow=nw, **fields), box, fields


def resize_center_crop(image, size, oh, ow, trimmed=True):
    """`Resize(size) -> CenterCrop((oh, ow))` -> (uint8 [oh, ow, 3], box, fields); `trimmed`: the box holds only what the taps read"""
    h, w = image.shape[:2]
    nh, nw = resized_hw(h, w, size)
    top, left = center_origin(nh, nw, oh, ow)
    r0, rh, c0, cw = stored_box(h, w, nh, nw, top, left, oh, ow) if trimmed else (0, h, 0, w)
    box = np.ascontiguousarray(image[r0:r0 + rh, c0:c0 + cw])
    fields = dict(full_h=h, full_w=w, row0=r0, col0=c0, nh=nh, nw=nw, flip=False, top=top, left=left)
    return window(box, oh=oh, ow=ow, **fields), box, fields


def normalize(u8, mean, std):
    """uint8 [h, w, 3] -> float32 [3, h, w]: `Normalize(mean, std)(ToTensor()(img))`, float32 arithmetic as torch's"""
    x = u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    x = (x - np.asarray(mean, np.float32).reshape(3, 1, 1)) / np.asarray(std, np.float32).reshape(3, 1, 1)
    return x.astype(np.float32)
